"""Held objects, measured on one GPU (`profiles/held_time.log`).

    python tools/held_time.py [--out profiles/held_time.log] [--reps 5] [--rows 1000000] [--edges 100000]

The c2 and c3 arms with the box of the parity fixtures in the hand (half extents 0.1, 0.1, 0.2, margin 0.04, 0.25 m along the
gripper's z; H = 1), its world copy parked out of reach.  Timing as tools/cloud_time.py: one HIP event pair around a window of
back-to-back calls sized to about 50 ms, a warm-up per shape, the median of --reps windows, the windows of the calls that are compared
alternating.
    validity    DeviceModel.held_validity at --rows configurations (packed words), with the stored grasp and with one grasp per row.
                Against it the one alternative the parent has: DeviceModel.validity on a descriptor that carries the same box as a
                robot shape of the gripper's frame with the same pairs ("box as link"), minus DeviceModel.validity on the plain
                scene.  The masks must agree: validity(box as link) == validity(plain) | held_validity.
    edges       DeviceModel.held_edge_validity at --edges edges a -> a + U(-0.5, 0.5), resolution 0.05, connect mode; against
                edge_validity on the box-as-link descriptor minus edge_validity on the plain scene; and the connector's sequence
                (edge_validity, then the held call ANDed into its result).  The valid flags must agree.
"""
import argparse
import dataclasses
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cloud_time import timed_pair, timed, fmt                                   # noqa: E402
from numbotics_amd.csrc.build import source_digest                               # noqa: E402
from numbotics_amd.engine import DeviceModel, held_locals                        # noqa: E402
from numbotics_amd.physics import Cuboid, World                                  # noqa: E402
from numbotics_amd.physics.world import _reset_worlds                            # noqa: E402
from numbotics_amd.scenes import build_scene, sample_q                           # noqa: E402


def box_as_link(sm, spec):
    """``sm`` with the held shapes as robot shapes of the holding frame and the held pairs behind the scene's own: the descriptor a
    caller of the parent had to build (and rebuild for every grasp)."""
    S, H = sm.n_rshapes, spec.n_shapes
    loc = held_locals(spec.A, spec.G, spec.shape_local).reshape(H, 12)
    pa = [int(s) for s in spec.robot_shapes for h in range(H)] + [S + h for h in range(H) for w in spec.world_shapes]
    pb = [S + h for s in spec.robot_shapes for h in range(H)] + [S + H + int(w) for h in range(H) for w in spec.world_shapes]
    return dataclasses.replace(
        sm, rshape_frame=np.concatenate((sm.rshape_frame, np.full(H, spec.frame))).astype(np.int32),
        rshape_type=np.concatenate((sm.rshape_type, spec.shape_type)).astype(np.int32),
        rshape_local=np.ascontiguousarray(np.concatenate((sm.rshape_local.reshape(S, 12), loc))),
        rshape_param=np.ascontiguousarray(np.concatenate((sm.rshape_param.reshape(S, 4), spec.shape_param))),
        rshape_link=np.concatenate((sm.rshape_link, np.zeros(H))).astype(np.int32),
        pair_a=np.concatenate((sm.pair_a, pa)).astype(np.int32),
        pair_b=np.concatenate((np.where(sm.pair_b >= S, sm.pair_b + H, sm.pair_b), pb)).astype(np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "held_time.log"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--edges", type=int, default=100000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/held_time.py needs a GPU: nothing is measured without one")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    log = open(args.out, "w")

    def say(line=""):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    say(f"# tools/held_time.py  build {source_digest()}  {torch.cuda.get_device_name(0)}  rows {args.rows}  edges {args.edges}  reps {args.reps}")
    for name in ("c2", "c3"):
        _reset_worlds()
        World()
        arm, chain, obs = build_scene(name)
        box = Cuboid(0.0, np.array([0.1, 0.1, 0.2]), collision_margin=0.04, position=np.array([0.0, 0.0, -6.0]))
        G = np.eye(4)
        G[2, 3] = 0.25
        att = arm.attach(box, "gripper", pose=G)
        sm, spec = arm.scene_model(), att.spec(arm)
        dev, held = att._device(arm)
        linked = DeviceModel(box_as_link(sm, spec))
        B, E = args.rows, args.edges
        qt = torch.from_numpy(sample_q(chain, B, seed=3)).cuda()
        say(f"## {name}: {sm.n_rshapes} robot shapes, {sm.n_wshapes} world shapes, {sm.n_pairs} pairs; held pairs: "
            f"{len(spec.world_shapes)} world + {len(spec.robot_shapes)} robot")
        # ---- validity
        own = dev.validity(qt, 0.0, packed=True)
        both = linked.validity(qt, 0.0, packed=True)
        alone = dev.held_validity(held, qt, 0.0, packed=True)
        if not torch.equal(both, own | alone):
            raise SystemExit(f"{name}: validity(box as link) != validity(plain) | held_validity")
        hits = sum(bin(int(w) & 0xFFFFFFFFFFFFFFFF).count("1") for w in alone.cpu().numpy()[:1000])
        say(f"validity  B = {B}: masks agree; the held object collides in {hits / 64000.0:.3f} of the first 64000 rows")
        t_held, t_link = timed_pair(lambda: dev.held_validity(held, qt, 0.0, packed=True), lambda: linked.validity(qt, 0.0, packed=True), args.reps)
        t_plain, t_link2 = timed_pair(lambda: dev.validity(qt, 0.0, packed=True), lambda: linked.validity(qt, 0.0, packed=True), args.reps)
        say(f"  held_validity (stored grasp)        {fmt(t_held)}")
        say(f"  validity, box as link               {fmt(t_link)}")
        say(f"  validity, box as link (2nd pairing) {fmt(t_link2)}")
        say(f"  validity, plain scene               {fmt(t_plain)}")
        say(f"  box as link minus plain             {t_link2[0] - t_plain[0]:9.3f} ms   (held_validity / that: {t_held[0] / max(t_link2[0] - t_plain[0], 1e-9):.2f})")
        Gt = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(G, (B, 4, 4)))).cuda()
        say(f"  held_validity (a grasp per row)     {fmt(timed(lambda: dev.held_validity(held, qt, 0.0, packed=True, pose=Gt), args.reps))}")
        mask = dev.validity(qt, 0.0, packed=True)
        say(f"  validity then held_validity(out=)   {fmt(timed(lambda: dev.held_validity(held, qt, 0.0, packed=True, out=dev.validity(qt, 0.0, packed=True)), args.reps))}")
        del Gt, mask
        # ---- edges
        rng = np.random.default_rng(5)
        st = qt[:E].contiguous()
        gt = st + torch.from_numpy(rng.uniform(-0.5, 0.5, (E, chain.dof))).cuda()
        ws = torch.empty((dev.held_edge_workspace_bytes(E),), dtype=torch.uint8, device="cuda")
        v_own, _, ns = dev.edge_validity(st, gt, 0.05, 10.0)
        v_both = linked.edge_validity(st, gt, 0.05, 10.0)[0]
        v_held = dev.held_edge_validity(held, st, gt, 0.05, 10.0, workspace=ws)[0]
        if not torch.equal(v_both, v_own & v_held):
            raise SystemExit(f"{name}: edge_validity(box as link) != edge_validity(plain) & held_edge_validity")
        say(f"edges  E = {E}, {int(ns.sum())} samples: flags agree; valid {float(v_held.float().mean()):.3f} (held alone), {float(v_both.float().mean()):.3f} (with the scene)")
        t_held, t_link = timed_pair(lambda: dev.held_edge_validity(held, st, gt, 0.05, 10.0, workspace=ws), lambda: linked.edge_validity(st, gt, 0.05, 10.0), args.reps)
        t_plain, t_link2 = timed_pair(lambda: dev.edge_validity(st, gt, 0.05, 10.0), lambda: linked.edge_validity(st, gt, 0.05, 10.0), args.reps)
        say(f"  held_edge_validity                  {fmt(t_held)}")
        say(f"  edge_validity, box as link          {fmt(t_link)}")
        say(f"  edge_validity, box as link (2nd)    {fmt(t_link2)}")
        say(f"  edge_validity, plain scene          {fmt(t_plain)}")
        say(f"  box as link minus plain             {t_link2[0] - t_plain[0]:9.3f} ms   (held_edge_validity / that: {t_held[0] / max(t_link2[0] - t_plain[0], 1e-9):.2f})")

        def sequence():
            res = dev.edge_validity(st, gt, 0.05, 10.0)
            dev.held_edge_validity(held, st, gt, 0.05, 10.0, out=res[0], workspace=ws)
        say(f"  edge_validity then held(out=)       {fmt(timed(sequence, args.reps))}")
        del linked, held, dev, qt, st, gt, ws
    log.close()


if __name__ == "__main__":
    main()
