"""Held objects, measured on one GPU (`profiles/held_time.log`).

    python tools/held_time.py [--out profiles/held_time.log] [--reps 5] [--rows 1000000] [--edges 100000] [--only records] [--mesh] [--mesh-cloud]

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
    trajectories  held_distances at --rows configurations, held_edge_continuous at --edges edges, held_spline_continuous and
                held_spline_validity at --splines trajectories (6 control points, degree 3, a random walk of step 0.12 from a sampled
                configuration).  The yardstick is the scene's own entry on the same inputs in the same process (pair_distances,
                edge_continuous, spline_continuous, spline_validity), per held item against per scene pair.  Each accumulated
                result must equal the scene's entry on the box-as-link descriptor, bit for bit.
    --only records  (log: profiles/held_records_time.log) nothing of the above but the record entries at --rows configurations:
                held_records (every item: distance, witness, gradient row), the same without rows and without either, and
                held_closest_records (held_distances, the argmin on the device, the listed record kernel), each beside
                held_distances on the same inputs.  Distances, witnesses and rows must equal the held columns of
                proximity_jacobian on the box-as-link descriptor, bit for bit.
    --mesh      (log: profiles/held_mesh_time.log) nothing of the above but what a held hull costs against the same object as a held
                box: DeviceModel.held_validity at --rows configurations of c2 (packed words) with the package's rock.obj in the
                gripper (``attach(..., meshes=True)``: one hull of 38 vertices and 72 planes, Bullet's 0.001 margin, 0.22 m along the
                gripper's z) beside the box of the parity fixtures, the windows of the two alternating; then held_distances of
                both at 65536 rows.  The hull's mask must equal validity(rock as link) with validity(plain) taken out of it, on
                a descriptor that carries the hull as a robot shape of the gripper's frame with the hull appended to its tables.
    --mesh-cloud  (log: profiles/held_mesh_cloud_time.log) nothing of the above but what a held hull costs against a scan: the rock
                (``attach(..., meshes=True, mesh_scans=True)``) beside the parity box on c2, against the dense scan of
                tools/cloud_time.py at 1e5 points (scan(N, seed=N), radius 0.01), the windows of the two alternating:
                DeviceModel.held_cloud_validity at --rows configurations (packed words), held_cloud_clearance at --rows / 10
                (d_max 0.05), and held_cloud_edge_continuous at --ca-edges edges a -> a + U(-0.5, 0.5) (connect mode, look_ahead
                0.05).  The rock's verdicts must equal cloud_validity of the rock-as-link descriptor selected on that one shape,
                and its clearance that descriptor's cloud_clearance, bit for bit.
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


def mesh(say, args):
    """The --mesh section: the rock in the gripper beside the parity box, on c2."""
    from numbotics_amd.physics import Mesh
    from numbotics_amd.scenes import MESH_DIR
    _reset_worlds()
    World()
    arm, chain, obs = build_scene("c2")
    park = np.array([0.0, 0.0, -6.0])
    box = Cuboid(0.0, np.array([0.1, 0.1, 0.2]), collision_margin=0.04, position=park.copy())
    rock = Mesh(0.0, os.path.join(MESH_DIR, "rock.obj"), position=park + np.array([0.0, 1.0, 0.0]))
    Gb, Gr = np.eye(4), np.eye(4)
    Gb[2, 3], Gr[2, 3] = 0.25, 0.22
    att_b = arm.attach(box, "gripper", pose=Gb)
    att_r = arm.attach(rock, "gripper", pose=Gr, meshes=True)
    sm, sb, sr = arm.scene_model(), att_b.spec(arm), att_r.spec(arm)
    dev, held_b = att_b._device(arm)
    _, held_r = att_r._device(arm)
    B = args.rows
    qt = torch.from_numpy(sample_q(chain, B, seed=3)).cuda()
    say(f"## c2 --mesh: {sm.n_rshapes} robot shapes, {sm.n_wshapes} world shapes; rock.obj: {sr.n_shapes} hull, "
        f"{int(sr.hull_vert_begin[-1])} vertices, {int(sr.hull_face_begin[-1])} planes, margin {float(sr.shape_param[0][3])}; held pairs "
        f"of either: {len(sr.world_shapes)} world + {len(sr.robot_shapes)} robot")
    # the rock as a link shape: the held hull behind the scene's hulls, its index shifted
    sp = sr.shape_param.copy()
    sp[:, 0] += sm.n_hulls
    as_link = box_as_link(sm, dataclasses.replace(sr, shape_param=sp))
    as_link = dataclasses.replace(
        as_link, hull_vert_begin=np.concatenate((sm.hull_vert_begin, sm.hull_vert_begin[-1] + sr.hull_vert_begin[1:])).astype(np.int32),
        hull_verts=np.ascontiguousarray(np.concatenate((sm.hull_verts.reshape(-1, 3), sr.hull_verts))),
        hull_face_begin=np.concatenate((sm.hull_face_begin, sm.hull_face_begin[-1] + sr.hull_face_begin[1:])).astype(np.int32),
        hull_planes=np.ascontiguousarray(np.concatenate((sm.hull_planes.reshape(-1, 4), sr.hull_planes))))
    linked = DeviceModel(as_link)
    own = dev.validity(qt, 0.0, packed=True)
    alone = dev.held_validity(held_r, qt, 0.0, packed=True)
    if not torch.equal(linked.validity(qt, 0.0, packed=True), own | alone):
        raise SystemExit("validity(rock as link) != validity(plain) | held_validity(rock)")
    share = lambda w: sum(bin(int(v) & 0xFFFFFFFFFFFFFFFF).count("1") for v in w.cpu().numpy()[:1000]) / 64000.0      # noqa: E731
    say(f"validity  B = {B}: masks agree; of the first 64000 rows the rock collides in {share(alone):.3f}, the box in "
        f"{share(dev.held_validity(held_b, qt, 0.0, packed=True)):.3f}")
    t_r, t_b = timed_pair(lambda: dev.held_validity(held_r, qt, 0.0, packed=True), lambda: dev.held_validity(held_b, qt, 0.0, packed=True), args.reps)
    say(f"  held_validity, rock.obj (hull)      {fmt(t_r)}")
    say(f"  held_validity, parity box           {fmt(t_b)}   (hull / box: {t_r[0] / t_b[0]:.2f})")
    n = 65536
    d_r = dev.held_distances(held_r, qt[:n])
    if not torch.equal(d_r.view(torch.int64), linked.pair_distances(qt[:n])[:, sm.n_pairs:].contiguous().view(torch.int64)):
        raise SystemExit("held_distances(rock) != the held columns of pair_distances(rock as link)")
    t_r, t_b = timed_pair(lambda: dev.held_distances(held_r, qt[:n]), lambda: dev.held_distances(held_b, qt[:n]), args.reps)
    say(f"distances  B = {n}, K = {held_r.n_items} items of either: the rock's agree with pair_distances(rock as link)")
    say(f"  held_distances, rock.obj (hull)     {fmt(t_r)}")
    say(f"  held_distances, parity box          {fmt(t_b)}   (hull / box: {t_r[0] / t_b[0]:.2f})")


def mesh_cloud(say, args):
    """The --mesh-cloud section: the rock and the parity box against the dense scan at 1e5 points, on c2."""
    from cloud_time import scan, RADIUS, BOX
    from numbotics_amd.physics import Mesh, PointCloud
    from numbotics_amd.scenes import MESH_DIR
    _reset_worlds()
    World()
    arm, chain, obs = build_scene("c2")
    park = np.array([0.0, 0.0, -6.0])
    box = Cuboid(0.0, np.array([0.1, 0.1, 0.2]), collision_margin=0.04, position=park.copy())
    rock = Mesh(0.0, os.path.join(MESH_DIR, "rock.obj"), position=park + np.array([0.0, 1.0, 0.0]))
    Gb, Gr = np.eye(4), np.eye(4)
    Gb[2, 3], Gr[2, 3] = 0.25, 0.22
    att_b = arm.attach(box, "gripper", pose=Gb)
    att_r = arm.attach(rock, "gripper", pose=Gr, meshes=True, mesh_scans=True)
    sm, sr = arm.scene_model(), att_r.spec(arm)
    dev, held_b = att_b._device(arm)
    _, held_r = att_r._device(arm)
    N, B, E = 10 ** 5, args.rows, args.ca_edges
    cloud = PointCloud(torch.from_numpy(scan(N, seed=N)).cuda(), RADIUS, bounds=BOX)
    qt = torch.from_numpy(sample_q(chain, B, seed=3)).cuda()
    qc = qt[:B // 10].contiguous()
    say(f"## c2 --mesh-cloud: N = {N} points, radius {RADIUS}, cell {cloud.cell:.4f}; rock.obj: {sr.n_shapes} hull, "
        f"{int(sr.hull_vert_begin[-1])} vertices, {int(sr.hull_face_begin[-1])} planes, margin {float(sr.shape_param[0][3])}, bounding "
        f"radius {float(np.linalg.norm(sr.hull_verts, axis=1).max()):.3f}; the box: 0.1, 0.1, 0.2, margin 0.04, bounding radius 0.245")
    # the rock as a link shape of a descriptor with no pairs of its own beyond the scene's: cloud_validity / cloud_clearance selected on it
    sp = sr.shape_param.copy()
    sp[:, 0] += sm.n_hulls
    as_link = box_as_link(sm, dataclasses.replace(sr, shape_param=sp))
    as_link = dataclasses.replace(
        as_link, hull_vert_begin=np.concatenate((sm.hull_vert_begin, sm.hull_vert_begin[-1] + sr.hull_vert_begin[1:])).astype(np.int32),
        hull_verts=np.ascontiguousarray(np.concatenate((sm.hull_verts.reshape(-1, 3), sr.hull_verts))),
        hull_face_begin=np.concatenate((sm.hull_face_begin, sm.hull_face_begin[-1] + sr.hull_face_begin[1:])).astype(np.int32),
        hull_planes=np.ascontiguousarray(np.concatenate((sm.hull_planes.reshape(-1, 4), sr.hull_planes))))
    linked = DeviceModel(as_link)
    one = [sm.n_rshapes]
    mine = dev.held_cloud_validity(held_r, cloud, qt, 0.0, packed=True)
    if not torch.equal(mine, linked.cloud_validity(cloud, qt, 0.0, packed=True, shapes=one)):
        raise SystemExit("held_cloud_validity(rock) != cloud_validity(rock as link, that shape)")
    d, _, p = dev.held_cloud_clearance(held_r, cloud, qc, 0.05)
    dl, _, pl = linked.cloud_clearance(cloud, qc, 0.05, shapes=one)
    if not (torch.equal(d.view(torch.int64), dl.view(torch.int64)) and torch.equal(p, pl)):
        raise SystemExit("held_cloud_clearance(rock) != cloud_clearance(rock as link, that shape)")
    share = lambda w: sum(bin(int(v) & 0xFFFFFFFFFFFFFFFF).count("1") for v in w.cpu().numpy()[:1000]) / 64000.0      # noqa: E731
    say(f"validity  B = {B}: the rock's mask agrees with cloud_validity(rock as link); of the first 64000 rows the rock collides in "
        f"{share(mine):.3f}, the box in {share(dev.held_cloud_validity(held_b, cloud, qt, 0.0, packed=True)):.3f}")
    t_r, t_b = timed_pair(lambda: dev.held_cloud_validity(held_r, cloud, qt, 0.0, packed=True),
                          lambda: dev.held_cloud_validity(held_b, cloud, qt, 0.0, packed=True), args.reps)
    say(f"  held_cloud_validity, rock.obj (hull)      {fmt(t_r)}")
    say(f"  held_cloud_validity, parity box           {fmt(t_b)}   (hull / box: {t_r[0] / t_b[0]:.2f})")
    db = dev.held_cloud_clearance(held_b, cloud, qc, 0.05)[0]
    say(f"clearance  B = {B // 10}, d_max 0.05: the rock's agrees with cloud_clearance(rock as link); below d_max: rock "
        f"{float(torch.isfinite(d).float().mean()):.3f}, box {float(torch.isfinite(db).float().mean()):.3f}")
    t_r, t_b = timed_pair(lambda: dev.held_cloud_clearance(held_r, cloud, qc, 0.05), lambda: dev.held_cloud_clearance(held_b, cloud, qc, 0.05),
                          args.reps)
    say(f"  held_cloud_clearance, rock.obj (hull)     {fmt(t_r)}")
    say(f"  held_cloud_clearance, parity box          {fmt(t_b)}   (hull / box: {t_r[0] / t_b[0]:.2f})")
    rng = np.random.default_rng(5)
    st = qt[:E].contiguous()
    gt = st + torch.from_numpy(rng.uniform(-0.5, 0.5, (E, chain.dof))).cuda()
    cr = dev.held_cloud_edge_continuous(held_r, cloud, st, gt, 10.0, look_ahead=0.05)
    cb = dev.held_cloud_edge_continuous(held_b, cloud, st, gt, 10.0, look_ahead=0.05)
    shares = lambda c: "/".join(str(int((c[3] == k).sum())) for k in (0, 1, 2))      # noqa: E731
    say(f"certified edges  E = {E}, connect, look_ahead 0.05, max_iter 64: FREE/COLLISION/UNDECIDED rock {shares(cr)}, box {shares(cb)}")
    t_r, t_b = timed_pair(lambda: dev.held_cloud_edge_continuous(held_r, cloud, st, gt, 10.0, look_ahead=0.05),
                          lambda: dev.held_cloud_edge_continuous(held_b, cloud, st, gt, 10.0, look_ahead=0.05), args.reps)
    say(f"  held_cloud_edge_continuous, rock.obj      {fmt(t_r)}")
    say(f"  held_cloud_edge_continuous, parity box    {fmt(t_b)}   (hull / box: {t_r[0] / t_b[0]:.2f})")


def records(say, name, dev, held, linked, qt, P, reps):
    """The --only records section for one scene."""
    B, K, n = int(qt.shape[0]), held.n_items, 16384
    d, w, j = dev.held_records(held, qt[:n])
    ref = linked.proximity_jacobian(qt[:n])
    same = lambda a, b: torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))      # noqa: E731
    if not (same(d, ref[0][:, P:]) and same(w, ref[1][:, P:]) and same(j, ref[2][:, P:])):
        raise SystemExit(f"{name}: held_records != the held columns of proximity_jacobian(box as link)")
    if not same(d, dev.held_distances(held, qt[:n])):
        raise SystemExit(f"{name}: held_records' distances != held_distances")
    cd, ci, cw, cj = dev.held_closest_records(held, qt[:n])
    b = torch.arange(n, device="cuda")
    if not (same(cd, d.min(dim=1).values) and same(cw, w[b, ci.long()]) and same(cj, j[b, ci.long()])):
        raise SystemExit(f"{name}: held_closest_records != the dense record at the argmin")
    say(f"records  B = {B}, K = {K} held items: records agree with proximity_jacobian(box as link) on the first {n} rows")
    del d, w, j, ref, cd, ci, cw, cj
    base = lambda: dev.held_distances(held, qt)      # noqa: E731
    for what, fn in (("held_records (witness, rows)", lambda: dev.held_records(held, qt)),
                     ("held_records (witness)", lambda: dev.held_records(held, qt, jacobian=False)),
                     ("held_records (distance alone)", lambda: dev.held_records(held, qt, witness=False, jacobian=False)),
                     ("held_closest_records", lambda: dev.held_closest_records(held, qt))):
        t_r, t_d = timed_pair(fn, base, reps)
        say(f"  {what:<35} {fmt(t_r)}   ({1e3 * t_r[0] / K:.1f} us per item)")
        say(f"  {'held_distances beside it':<35} {fmt(t_d)}   (ratio {t_r[0] / t_d[0]:.2f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("records",), default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--edges", type=int, default=100000)
    ap.add_argument("--splines", type=int, default=10000)
    ap.add_argument("--mesh", action="store_true")
    ap.add_argument("--mesh-cloud", action="store_true")
    ap.add_argument("--ca-edges", type=int, default=1000)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "held_mesh_cloud_time.log" if args.mesh_cloud else "held_mesh_time.log" if args.mesh else
                                "held_records_time.log" if args.only == "records" else "held_time.log")
    if not torch.cuda.is_available():
        raise SystemExit("tools/held_time.py needs a GPU: nothing is measured without one")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    log = open(args.out, "w")

    def say(line=""):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    say(f"# tools/held_time.py  build {source_digest()}  {torch.cuda.get_device_name(0)}  rows {args.rows}  edges {args.edges}  reps {args.reps}")
    if args.mesh_cloud or args.mesh:
        (mesh_cloud if args.mesh_cloud else mesh)(say, args)
        log.close()
        return
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
        if args.only == "records":
            records(say, name, dev, held, linked, qt, sm.n_pairs, args.reps)
            del linked, held, dev, qt
            continue
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
        # ---- trajectories: distances, certified edges, certified and sampled splines; the yardstick is the scene's own entry on
        # the same inputs in the same process (the scene's P pairs against the held object's K items: ms per pair / per item)
        K, P, S = held.n_items, sm.n_pairs, args.splines
        d_held = dev.held_distances(held, qt)
        d_link = linked.pair_distances(qt[:65536])[:, P:]
        if not torch.equal(d_held[:65536].view(torch.int64), d_link.contiguous().view(torch.int64)):
            raise SystemExit(f"{name}: held_distances != the held columns of pair_distances(box as link)")
        del d_held, d_link
        say(f"trajectories  K = {K} held items, P = {P} scene pairs")
        t_d, t_pd = timed_pair(lambda: dev.held_distances(held, qt), lambda: dev.pair_distances(qt), args.reps)
        say(f"  held_distances, B = {B}              {fmt(t_d)}   ({1e3 * t_d[0] / K:.1f} us per item)")
        say(f"  pair_distances (scene), B = {B}      {fmt(t_pd)}   ({1e3 * t_pd[0] / P:.1f} us per pair; per item / per pair: {t_d[0] * P / (t_pd[0] * K):.2f})")
        c_own = dev.edge_continuous(st, gt, 10.0)
        c_held = dev.held_edge_continuous(held, st, gt, 10.0)
        c_both = linked.edge_continuous(st, gt, 10.0)
        acc = tuple(x.clone() for x in (c_own[0], c_own[2], c_own[3]))
        dev.held_edge_continuous(held, st, gt, 10.0, out=acc)
        if not (torch.equal(acc[2], c_both[3]) and torch.equal(acc[1].view(torch.int64), c_both[2].view(torch.int64))):
            raise SystemExit(f"{name}: edge_continuous then held_edge_continuous(out=) != edge_continuous(box as link)")
        say(f"certified edges  E = {E}: results agree; FREE {float((c_held[3] == 0).float().mean()):.3f} (held alone), "
            f"{float((c_both[3] == 0).float().mean()):.3f} (with the scene)")
        t_h, t_s = timed_pair(lambda: dev.held_edge_continuous(held, st, gt, 10.0), lambda: dev.edge_continuous(st, gt, 10.0), args.reps)
        say(f"  held_edge_continuous                {fmt(t_h)}   ({1e3 * t_h[0] / K:.1f} us per item)")
        say(f"  edge_continuous (scene)             {fmt(t_s)}   ({1e3 * t_s[0] / P:.1f} us per pair; per item / per pair: {t_h[0] * P / (t_s[0] * K):.2f})")

        def certified():
            r = dev.edge_continuous(st, gt, 10.0)
            dev.held_edge_continuous(held, st, gt, 10.0, out=(r[0], r[2], r[3]))
        say(f"  edge_continuous then held(out=)     {fmt(timed(certified, args.reps))}")
        from numbotics_amd.planning import unit_knots
        ctrl = qt[:S, None, :] + torch.cumsum(torch.from_numpy(np.random.default_rng(7).uniform(-0.12, 0.12, (S, 6, chain.dof))).cuda(), dim=1)
        ctrl = ctrl.contiguous()
        kn = unit_knots(6, 3)
        knt = torch.from_numpy(kn).cuda()
        s_held = dev.held_spline_continuous(held, ctrl, knt, 3)
        s_both = linked.spline_continuous(ctrl, knt, 3)
        acc = dev.spline_continuous(ctrl, knt, 3)
        dev.held_spline_continuous(held, ctrl, knt, 3, out=acc)
        if not (torch.equal(acc[2], s_both[2]) and torch.equal(acc[1].view(torch.int64), s_both[1].view(torch.int64))):
            raise SystemExit(f"{name}: spline_continuous then held_spline_continuous(out=) != spline_continuous(box as link)")
        say(f"certified splines  S = {S}, 6 control points, degree 3: results agree; FREE {float((s_held[2] == 0).float().mean()):.3f} "
            f"(held alone), {float((s_both[2] == 0).float().mean()):.3f} (with the scene)")
        t_h, t_s = timed_pair(lambda: dev.held_spline_continuous(held, ctrl, knt, 3), lambda: dev.spline_continuous(ctrl, knt, 3), args.reps)
        say(f"  held_spline_continuous              {fmt(t_h)}   ({1e3 * t_h[0] / K:.1f} us per item)")
        say(f"  spline_continuous (scene)           {fmt(t_s)}   ({1e3 * t_s[0] / P:.1f} us per pair; per item / per pair: {t_h[0] * P / (t_s[0] * K):.2f})")
        ws2 = torch.empty((dev.held_spline_workspace_bytes(S),), dtype=torch.uint8, device="cuda")
        v_held = dev.held_spline_validity(held, ctrl, knt, 3, 0.05, workspace=ws2)
        v_both = linked.spline_validity(ctrl, kn, 3, 0.05)
        acc = dev.spline_validity(ctrl, kn, 3, 0.05)
        dev.held_spline_validity(held, ctrl, knt, 3, 0.05, out=acc, workspace=ws2)
        if not (torch.equal(acc[0], v_both[0]) and torch.equal(acc[1].view(torch.int64), v_both[1].view(torch.int64))):
            raise SystemExit(f"{name}: spline_validity then held_spline_validity(out=) != spline_validity(box as link)")
        say(f"sampled splines  S = {S}, resolution 0.05, {int(v_held[2].sum())} samples: results agree; valid "
            f"{float(v_held[0].float().mean()):.3f} (held alone), {float(v_both[0].float().mean()):.3f} (with the scene)")
        t_h, t_s = timed_pair(lambda: dev.held_spline_validity(held, ctrl, knt, 3, 0.05, workspace=ws2),
                              lambda: dev.spline_validity(ctrl, kn, 3, 0.05), args.reps)
        say(f"  held_spline_validity                {fmt(t_h)}")
        say(f"  spline_validity (scene)             {fmt(t_s)}   (held / scene: {t_h[0] / t_s[0]:.2f})")
        del linked, held, dev, qt, st, gt, ws, ws2, ctrl, acc
    log.close()


if __name__ == "__main__":
    main()
