"""Moving world bodies, measured on one GPU (`profiles/r10_world_update.log`).

    python tools/world_update_time.py [--out profiles/r10_world_update.log]
        1. move + check: median wall time of "move one cube, then in_collision on a resident batch" on c3, B = 4 096 and 1e6,
           200 moves after 20 warm-up moves, (a) Arm(chain) -- every move rebuilds the device scene -- and (b)
           Arm(chain, movable_world=True), same process, same moves.
        2. steady state: validity on 1e6 q of c2 at unchanged poses, ordinary descriptor (A) against a movable one (B) whose
           radius leaves the float32 slack as it is, interleaved, 20 batches each, next to A against A; then B with 4 x the
           radius (a more conservative broadphase: queue items per configuration from the device counters are not read here --
           the kernel trace of a profiler run has the k_narrow* times).
    python tools/world_update_time.py --update-only c3 | many
        400 updates of c3 (W = 8) or of 1 000 random obstacles, nothing else: run it under a kernel-trace profiler (its own
        run, no counters) for the duration of k_world_update.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from numbotics_amd.engine import DeviceModel  # noqa: E402
from numbotics_amd.physics import World, GraphChain  # noqa: E402
from numbotics_amd.physics.world import _reset_worlds  # noqa: E402
from numbotics_amd.robots import Arm  # noqa: E402
from numbotics_amd.scenes import build_scene, sample_q, apply_rrt_script_removals, KINOVA_URDF  # noqa: E402

LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def c3(movable):
    _reset_worlds()
    World()
    _, chain, obs = build_scene("c3")
    arm = Arm(chain, movable_world=movable)
    apply_rrt_script_removals(arm)
    return arm, chain, obs


def move_and_check(movable, B, moves=200, warm=20):
    arm, chain, obs = c3(movable)
    q = torch.from_numpy(sample_q(chain, B, seed=1)).cuda()
    rng = np.random.default_rng(3)
    steps = rng.uniform(-0.02, 0.02, (moves + warm, 3))
    arm.in_collision(q)
    torch.cuda.synchronize()
    times, handles = [], set()
    for i in range(moves + warm):
        cube = obs[i % len(obs)]
        t0 = time.perf_counter()
        cube.position = cube.position + steps[i]
        m = arm.in_collision(q)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if i >= warm:
            times.append(dt)
            handles.add(arm._scene_device()[1]._h.value)
    return statistics.median(times) * 1e3, min(times) * 1e3, max(times) * 1e3, len(handles), float(m.float().mean())


def timed_validity(dev, q, n=20):
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dev.validity(q, 0.0, packed=True)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def steady_state():
    _reset_worlds()
    World()
    arm, chain, obs = build_scene("c2")
    sm = arm.scene_model()
    q = torch.from_numpy(sample_q(chain, 1_000_000, seed=1)).cuda()
    k = sm.kin
    reach = float(np.sum(np.linalg.norm(np.asarray(k.joint_trans).reshape(-1, 3), axis=1)))
    far = float(np.max(np.linalg.norm(sm.wshape_pose.reshape(-1, 3, 4)[:, :, 3], axis=1)))
    tight = max(reach, far)
    A, A2 = DeviceModel(sm), DeviceModel(sm)
    Bm = DeviceModel(sm, movable=True, world_radius=tight)
    B4 = DeviceModel(sm, movable=True, world_radius=4.0 * tight)
    devs = {"A ordinary": A, "A' ordinary": A2, "B movable, radius = reach": Bm, "B4 movable, radius = 4 x reach": B4}
    for d in devs.values():
        for _ in range(3):
            d.validity(q, 0.0, packed=True)
    torch.cuda.synchronize()
    times = {name: [] for name in devs}
    for _ in range(20):                                  # interleaved: one batch each, round robin
        for name, d in devs.items():
            times[name] += timed_validity(d, q, 1)
    say("steady state, c2, 1e6 q, threshold 0, 20 interleaved batches each (ms: median, min, max); radius = %.3f m" % tight)
    for name, t in times.items():
        say("  %-32s %.4f  %.4f  %.4f   broadphase kernel %d" % (name, statistics.median(t), min(t), max(t), devs[name].broad_kernel_used()))
    ref = A.validity(q, 0.0)
    for name, d in devs.items():
        assert torch.equal(d.validity(q, 0.0), ref), name
    say("  masks of all four equal")


def update_only(which):
    from random_scenes import random_obstacles
    if which == "c3":
        arm, chain, keep = c3(True)
    else:
        _reset_worlds()
        World()
        chain = GraphChain.from_urdf(KINOVA_URDF)
        arm = Arm(chain, movable_world=True)
        keep = random_obstacles(np.random.default_rng(31), 1000, reach=2.5)
    sm, dev = arm._scene_device()
    P = torch.from_numpy(sm.wshape_pose).cuda()
    for _ in range(200):
        dev.set_world_poses(P)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        dev.set_world_poses(P)
    torch.cuda.synchronize()
    print("W = %d, %d pairs: %.2f us per update (host issue + device, back to back), status %d"
          % (sm.n_wshapes, sm.n_pairs, (time.perf_counter() - t0) / 200 * 1e6, dev.world_status()), flush=True)
    del keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--update-only", choices=("c3", "many"), default=None)
    a = ap.parse_args()
    if a.update_only:
        update_only(a.update_only)
        return
    say("device: %s" % torch.cuda.get_device_name(0))
    say("move one cube of c3, then in_collision on a resident batch; 200 moves after 20 warm-up (ms: median, min, max)")
    for B in (4096, 1_000_000):
        ra = move_and_check(False, B)
        rb = move_and_check(True, B)
        say("  B = %7d  (a) rebuild per move   %.3f  %.3f  %.3f   descriptors seen %d, colliding %.3f" % ((B,) + ra))
        say("  B = %7d  (b) movable_world=True %.3f  %.3f  %.3f   descriptors seen %d, colliding %.3f" % ((B,) + rb))
        say("  B = %7d  (a) / (b) = %.1f" % (B, ra[0] / rb[0]))
    steady_state()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
