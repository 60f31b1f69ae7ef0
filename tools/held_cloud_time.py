"""The held object against point clouds, measured on one GPU (`profiles/held_cloud_time.log`).

    python tools/held_cloud_time.py [--out profiles/held_cloud_time.log] [--reps 5] [--rows 1000000] [--only records]

Scene c2 with the box of the parity fixtures in the hand (half extents 0.1, 0.1, 0.2, margin 0.04, 0.25 m along the gripper's z;
H = 1), against the scans of tools/cloud_time.py (scan(N, seed=N), radius 0.01, N = 1e3 and 1e5).  Timing as tools/cloud_time.py:
one HIP event pair around a window of back-to-back calls sized to about 50 ms, a warm-up per shape, the median of --reps windows,
the windows of the two calls that are compared alternating; the calls of a window rotate over three batches of configurations.
    validity    DeviceModel.held_cloud_validity at --rows configurations (packed words) next to
                DeviceModel.cloud_validity(shapes=[one box shape of the gripper]) on the same inputs: the same grid walk for one
                shape of the same kind, by code the held walk does not share.  Beyond it the held walk forms two 3x4 products per
                lane, so a ratio near 1 is expected; beyond about 1.5 something other than the walk is being paid for.
    clearance   DeviceModel.held_cloud_clearance next to DeviceModel.cloud_clearance(shapes=[that shape]) at --rows / 10, d_max 0.05.
The held box is larger than the gripper's and stands elsewhere, so those two calls meet different numbers of points.  The lines
marked "twin" take that out: a held box of the gripper box's own size and margin, grasped so that it stands exactly where the
gripper box stands -- the same questions, asked through the two walks.  Their masks are compared (the two local poses are formed by
different products, so single rows may differ in the last bits; the count of differing rows is printed).
    --only records  (log: profiles/held_cloud_records_time.log) nothing of the above but DeviceModel.held_cloud_records at --rows / 10,
                d_max 0.05 -- with witness and rows, with the witness alone, with neither -- each beside held_cloud_clearance on the
                same inputs, whose distance, shape and point it must repeat bit for bit.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cloud_time import timed_pair, fmt, scan, RADIUS, BOX                          # noqa: E402
from numbotics_amd.csrc.build import source_digest                               # noqa: E402
from numbotics_amd.physics import Cuboid, PointCloud                             # noqa: E402
from numbotics_amd.scenes import build_scene, sample_q                           # noqa: E402

SH_BOX = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("records",), default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1000000)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "held_cloud_records_time.log" if args.only == "records" else "held_cloud_time.log")
    if not torch.cuda.is_available():
        raise SystemExit("tools/held_cloud_time.py needs a GPU: nothing is measured without one")
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
    sm, spec = arm.scene_model(), att.spec(arm)
    # the gripper's box: the last box shape on the holding frame (the base of the two-finger gripper)
    boxes = [s for s in range(sm.n_rshapes) if sm.rshape_frame[s] == spec.frame and sm.rshape_type[s] == SH_BOX]
    if not boxes:
        raise SystemExit("the holding frame of c2 carries no box shape to compare with")
    one = [boxes[-1]]
    # the twin: the gripper box once more, as a held object (its parked world copy changes the scene: both attachments are resolved
    # against the descriptor made after it)
    par = sm.rshape_param.reshape(-1, 4)[one[0]]
    L = np.eye(4)
    L[:3] = sm.rshape_local.reshape(-1, 3, 4)[one[0]]
    A = np.eye(4)
    A[:3] = np.asarray(spec.A, dtype=np.float64).reshape(-1, 4)[:3]
    twin_box = Cuboid(0.0, par[:3].copy(), collision_margin=float(par[3]), position=np.array([0.0, 0.0, -7.0]))
    twin_att = arm.attach(twin_box, "gripper", pose=np.linalg.inv(A) @ L)
    sm = arm.scene_model()
    dev, held = att._device(arm)
    twin = twin_att._device(arm)[1]
    assert twin.dev is dev and held.dev is dev
    B = args.rows
    say(f"# tools/held_cloud_time.py  build {source_digest()}  {torch.cuda.get_device_name(0)}  rows {B}  reps {args.reps}  radius {RADIUS}")
    say(f"# the shape compared with: robot shape {one[0]} of c2 (a box of {sm.links[sm.rshape_link[one[0]]]._name}, half extents "
        f"{[round(float(v), 4) for v in sm.rshape_param.reshape(-1, 4)[one[0]][:3]]}); the held box: 0.1, 0.1, 0.2, margin 0.04")
    qs = [torch.from_numpy(sample_q(chain, B, seed=2 + k)).cuda() for k in range(3)]
    qc = [q[:B // 10].contiguous() for q in qs]
    Gt = torch.from_numpy(G).cuda()
    turn = [0]

    def rotating(fn, batches):
        def call():
            turn[0] += 1
            return fn(batches[turn[0] % len(batches)])
        return call

    for N in (10 ** 3, 10 ** 5):
        cloud = PointCloud(torch.from_numpy(scan(N, seed=N)).cuda(), RADIUS, bounds=BOX)
        say(f"## N = {N}: cell {cloud.cell:.4f}, grid {tuple(int(d) for d in cloud.dims)}")
        if args.only == "records":
            d, s, p = dev.held_cloud_clearance(held, cloud, qc[0], 0.05)
            rd, rs, rp, rw, rj = dev.held_cloud_records(held, cloud, qc[0], 0.05)
            if not (torch.equal(d.view(torch.int64), rd.view(torch.int64)) and torch.equal(s, rs) and torch.equal(p, rp)):
                raise SystemExit("held_cloud_records' distance, shape and point != held_cloud_clearance's")
            win = s >= 0
            if not (torch.isfinite(rw[win]).all() and torch.isnan(rw[~win]).all() and not rj[~win].any()):
                raise SystemExit("held_cloud_records: a winner without a witness, or a loser with one or with a row")
            say(f"records  B = {B // 10}, d_max 0.05: below d_max {float(win.float().mean()):.3f}; distance, shape and point are held_cloud_clearance's")
            del d, s, p, rd, rs, rp, rw, rj
            clear = rotating(lambda q: dev.held_cloud_clearance(held, cloud, q, 0.05), qc)
            for what, kw in (("held_cloud_records (witness, rows)", dict()), ("held_cloud_records (witness)", dict(jacobian=False)),
                             ("held_cloud_records (neither)", dict(witness=False, jacobian=False))):
                t_r, t_c = timed_pair(rotating(lambda q, kw=kw: dev.held_cloud_records(held, cloud, q, 0.05, **kw), qc), clear, args.reps)
                say(f"  {what:<35} {fmt(t_r)}")
                say(f"  {'held_cloud_clearance beside it':<35} {fmt(t_c)}   (ratio {t_r[0] / t_c[0]:.2f})")
            del cloud
            continue
        mine = dev.held_cloud_validity(held, cloud, qs[0], 0.0, packed=True)
        if not torch.equal(mine, dev.held_cloud_validity(held, cloud, qs[0], 0.0, packed=True, pose=Gt)):
            raise SystemExit("the stored grasp and the same grasp given with the call disagree")
        other = dev.cloud_validity(cloud, qs[0], 0.0, packed=True, shapes=one)
        hits = lambda w: sum(bin(int(v) & 0xFFFFFFFFFFFFFFFF).count("1") for v in w.cpu().numpy()[:1000]) / 64000.0      # noqa: E731
        say(f"validity  B = {B}: colliding in the first 64000 rows: held box {hits(mine):.3f}, gripper box {hits(other):.3f}")
        t_h, t_c = timed_pair(rotating(lambda q: dev.held_cloud_validity(held, cloud, q, 0.0, packed=True), qs),
                              rotating(lambda q: dev.cloud_validity(cloud, q, 0.0, packed=True, shapes=one), qs), args.reps)
        say(f"  held_cloud_validity                 {fmt(t_h)}")
        say(f"  cloud_validity, one gripper box     {fmt(t_c)}")
        say(f"  ratio held / cloud                  {t_h[0] / t_c[0]:9.2f}")
        tw = dev.held_cloud_validity(twin, cloud, qs[0], 0.0, packed=True)
        diff = sum(bin(int(v) & 0xFFFFFFFFFFFFFFFF).count("1") for v in (tw ^ other).cpu().numpy())
        t_h, t_c = timed_pair(rotating(lambda q: dev.held_cloud_validity(twin, cloud, q, 0.0, packed=True), qs),
                              rotating(lambda q: dev.cloud_validity(cloud, q, 0.0, packed=True, shapes=one), qs), args.reps)
        say(f"  twin: held_cloud_validity           {fmt(t_h)}   ({diff} of {B} rows differ from the gripper box's)")
        say(f"  twin: cloud_validity                {fmt(t_c)}")
        say(f"  twin: ratio held / cloud            {t_h[0] / t_c[0]:9.2f}")
        d, _, _ = dev.held_cloud_clearance(held, cloud, qc[0], 0.05)
        dc, _, _ = dev.cloud_clearance(cloud, qc[0], 0.05, shapes=one)
        say(f"clearance  B = {B // 10}, d_max 0.05: below d_max: held box {float(torch.isfinite(d).float().mean()):.3f}, "
            f"gripper box {float(torch.isfinite(dc).float().mean()):.3f}")
        t_h, t_c = timed_pair(rotating(lambda q: dev.held_cloud_clearance(held, cloud, q, 0.05), qc),
                              rotating(lambda q: dev.cloud_clearance(cloud, q, 0.05, shapes=one), qc), args.reps)
        say(f"  held_cloud_clearance                {fmt(t_h)}")
        say(f"  cloud_clearance, one gripper box    {fmt(t_c)}")
        say(f"  ratio held / cloud                  {t_h[0] / t_c[0]:9.2f}")
        t_h, t_c = timed_pair(rotating(lambda q: dev.held_cloud_clearance(twin, cloud, q, 0.05), qc),
                              rotating(lambda q: dev.cloud_clearance(cloud, q, 0.05, shapes=one), qc), args.reps)
        say(f"  twin: held_cloud_clearance          {fmt(t_h)}")
        say(f"  twin: cloud_clearance               {fmt(t_c)}")
        say(f"  twin: ratio held / cloud            {t_h[0] / t_c[0]:9.2f}")
        del cloud
    log.close()
    del obs, box, twin_box


if __name__ == "__main__":
    main()
