"""Shared pieces of the per-robot broadphase tests (test_broad_spec_source.py on the CPU, test_broad_spec.py on the GPU): the fixed
list of generated robots that spans the Spec space, the generated source and its parser, an independent restatement of ``struct Spec``
from the scene model, and the check that a call was served by the specialised kernel."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np

GENERIC, SPECIALISED = 1, 2
THRESHOLDS = (0.0, 1e-6, 0.01, -0.002)
SPEC_MIN_BATCH = 1 << 16
FUZZ_B = SPEC_MIN_BATCH + 37
# core kinds of the device (nbk_device.hpp: point, segment, box, cylinder, hull, plane) by the model's shape type
CORE_KIND = {0: 0, 1: 1, 2: 2, 3: 3, 4: 5, 5: 4}
JK_GENERIC, JK_PRISMATIC = 3, 4

# (moving joints, robot shapes, axis mode, shapes on the base, fixed joints, obstacles).  The case's index is its seed; odd seeds use
# sharp shapes (bullet_margins=False).  Cases with index % 5 in (1, 3) get pair removals (see build_case).
SPEC_CASES = (
    (1, 1, "prismatic", False, 0, ("box",)),
    (1, 2, "aligned", True, 0, ("sphere", "capsule")),
    (2, 2, "aligned", True, 0, ()),
    (2, 7, "mixed", True, 1, ("capsule", "box")),
    (2, 8, "random", False, 1, ("plane",)),
    (7, 7, "aligned", False, 0, ("box", "cylinder")),
    (7, 9, "mixed", True, 2, ("cylinder", "plane")),
    (7, 12, "random", True, 0, ("mesh",)),
    (7, 13, "prismatic", False, 3, ("plane", "mesh")),
    (7, 15, "mixed", True, 1, ("sphere",)),
    (7, 16, "aligned", True, 2, ("mesh", "sphere")),
    (8, 8, "mixed", False, 0, ("cylinder",)),
    (8, 9, "aligned", True, 1, ()),
    (8, 12, "mixed", False, 2, ("capsule",)),
    (8, 13, "mixed", True, 0, ("plane", "mesh")),
    (8, 15, "random", True, 4, ("box",)),
    (8, 16, "mixed", True, 0, ("capsule", "plane")),
    (3, 4, "aligned", True, 0, ("cylinder",)),
    (4, 6, "prismatic", True, 1, ("sphere", "mesh")),
    (5, 10, "mixed", False, 2, ("cylinder", "box")),
    (6, 11, "random", True, 1, ("mesh",)),
    (6, 14, "aligned", False, 0, ("plane", "capsule")),
    (3, 3, "mixed", True, 0, ()),
    (4, 5, "aligned", False, 1, ("sphere", "sphere")),
    (5, 12, "mixed", True, 0, ("box", "mesh")),
    (6, 16, "random", False, 3, ("cylinder",)),
    (2, 2, "prismatic", False, 0, ("plane",)),
    (8, 16, "aligned", False, 3, ("mesh", "cylinder")),
    (4, 9, "mixed", True, 2, ("capsule", "capsule")),
    (7, 8, "mixed", True, 0, ("box", "plane")),
)
# the generated robot of the input-edge tests: prismatic joints, S >= 13, two world shapes that are not boxes
EDGE_CASE = 14
NAMED_CASES = ("c2", "c2m", "plane_hull")


def lib():
    """libnbk with the prototypes numbotics_amd._lib declares."""
    from numbotics_amd import _lib as L
    return L.load()


def fresh():
    from numbotics_amd.physics import World
    from numbotics_amd.physics.world import _reset_worlds
    _reset_worlds()
    World()


def has_removals(idx):
    return idx % 5 in (1, 3)


def build_case(idx, tmp):
    """-> (arm, chain, obstacles) of generated case ``idx`` in a fresh world; the same in every process."""
    from numbotics_amd.physics import GraphChain
    from numbotics_amd.robots import Arm
    from random_scenes import random_spec_robot, spec_obstacles
    n_joints, n_shapes, mode, base, fixed, kinds = SPEC_CASES[idx]
    fresh()
    rng = np.random.default_rng(1000 + idx)
    path = random_spec_robot(rng, os.path.join(tmp, f"spec_case_{idx}.urdf"), n_joints=n_joints, n_shapes=n_shapes, axis_mode=mode,
                             base_shapes=base, fixed_joints=fixed)
    chain = GraphChain.from_urdf(path)
    arm = Arm(chain, bullet_margins=idx % 2 == 0)
    reach = 0.12 * min(n_joints, 4) + 0.08
    obs = spec_obstacles(rng, kinds, reach, mesh_dir=tmp)
    if has_removals(idx):
        shaped = [l for l in chain._links if l._collision_shapes]
        # the first obstacle keeps its pairs with every second shaped link only
        if obs and len(shaped) >= 2:
            for link in shaped[1::2]:
                arm.remove_collision_pair(link, obs[0])
        # a handful of self pairs go, so that rows and slot groups of the robot-robot table hold one pair or none
        self_pairs = arm._sorted_pairs(arm.self_collision_pairs())
        if len(self_pairs) > 4:
            for k in rng.permutation(len(self_pairs))[:min(4, len(self_pairs) // 3)]:
                arm.remove_collision_pair(*self_pairs[int(k)])
            self_pairs = arm._sorted_pairs(arm.self_collision_pairs())
        # every self pair of the second shaped link goes: its rows of the robot-robot table are empty while later rows are not
        if idx % 5 == 3 and len(shaped) >= 4:
            for a, b in self_pairs:
                if shaped[1] in (a, b):
                    arm.remove_collision_pair(a, b)
        # a third obstacle none of whose pairs stays: the scene model lists a world shape with its first pair, so this one never
        # enters it (W stays 2); a descriptor with W = 3, NW = 2 is built by hand in test_broad_spec_source.py
        if len(obs) == 2:
            extra = spec_obstacles(rng, ("sphere",), reach, first=2)[0]
            for link in chain._links:
                arm.remove_collision_pair(link, extra)
            obs.append(extra)
    return arm, chain, obs


def named_case(name):
    """-> (arm, chain, obstacles) of c2 / c2m / plane_hull in a fresh world."""
    from numbotics_amd.scenes import build_scene
    fresh()
    if name == "plane_hull":
        from numbotics_amd.physics import GraphChain, Mesh, Plane
        from numbotics_amd.robots import Arm
        from numbotics_amd.scenes import KINOVA_URDF, MESH_DIR, apply_rrt_script_removals
        chain = GraphChain.from_urdf(KINOVA_URDF)
        arm = Arm(chain)
        apply_rrt_script_removals(arm)
        obs = [Plane(0.0, np.array([0.0, 0.0, 1.0]), position=np.array([0.0, 0.0, -0.3])),
               Mesh(0.0, os.path.join(MESH_DIR, "rock.obj"), position=np.array([0.55, 0.25, 0.45]))]
        return arm, chain, obs
    return build_scene(name)


def any_case(key, tmp):
    return build_case(key, tmp) if isinstance(key, int) else named_case(key)


def limits(chain):
    """Joint limits with continuous joints as [-pi, pi]."""
    lim = np.asarray(chain.joint_limits, dtype=np.float64)
    return np.where(np.isfinite(lim), lim, np.sign(lim) * np.pi)


def sample(chain, n, seed):
    lim = limits(chain)
    return np.random.default_rng(seed).uniform(lim[:, 0], lim[:, 1], (n, chain.dof))


def spec_source(sm):
    """-> (length or status, generated source or None) of a scene model; needs no device."""
    from numbotics_amd.engine import model_desc
    L = lib()
    d, keep = model_desc(sm)
    n = L.nbk_broad_spec_source(C.byref(d), None, 0)
    if n <= 0:
        return n, None
    buf = C.create_string_buffer(int(n))
    assert L.nbk_broad_spec_source(C.byref(d), buf, n) == n
    del keep
    return n, buf.value


def parse_spec(src):
    """The ``static constexpr`` members of the generated ``struct Spec`` -> dict (ints, bools and int lists)."""
    text = src.decode()
    text = text[text.index("struct Spec {"):]
    text = text[:text.index("\n};\n")]
    out = {}
    for line in text.splitlines():
        m = re.match(r"\s*static constexpr int (\w+)\[\] = \{([^}]*)\};", line)
        if m:
            out[m.group(1)] = [int(v) for v in m.group(2).split(",")]
            continue
        m = re.match(r"\s*static constexpr (int|bool) ((?:\w+ = [\w-]+(?:, )?)+);", line)
        if m:
            for item in m.group(2).split(", "):
                k, v = item.split(" = ")
                out[k] = (v == "true") if m.group(1) == "bool" else int(v)
    return out


def expected_spec(sm):
    """What ``struct Spec`` must say, restated from the SceneModel arrays alone (robots/model.py).  The device lists robot shapes
    by frame (base first, ties in model order), so shape s of the model is slot ``slot[s]`` there."""
    kin = sm.kin
    S, J = sm.n_rshapes, kin.n_joints
    by_frame = sorted(range(S), key=lambda s: (int(sm.rshape_frame[s]), s))
    slot = {s: i for i, s in enumerate(by_frame)}
    begin = [0]
    for f in range(-1, J):
        begin.append(begin[-1] + int(np.sum(sm.rshape_frame == f)))
    jkind = []
    for k in range(J):
        if kin.joint_type[k] == 1:
            jkind.append(JK_PRISMATIC)
            continue
        a = np.abs(kin.joint_axis[k])
        unit = [e for e in range(3) if a[e] == 1.0 and a[(e + 1) % 3] == 0.0 and a[(e + 2) % 3] == 0.0]
        jkind.append(unit[0] if unit else JK_GENERIC)
    rr, rw = set(), set()
    for a, b in zip(sm.pair_a.tolist(), sm.pair_b.tolist()):
        if b < S:
            x, y = slot[a], slot[b]
            rr.add((min(x, y), max(x, y)))
        else:
            rw.add((b - S, slot[a]))
    wl = sorted({w for w, _ in rw})
    return dict(S=S, SB=8 if S <= 8 else (12 if S <= 12 else 16), NQ=kin.n_q, J=J, W=sm.n_wshapes, NW=len(wl),
                qcol=[int(v) for v in kin.joint_qidx], sh_begin=begin, jkind=jkind, wl=wl,
                wk=[CORE_KIND[int(sm.wshape_type[w])] for w in wl], rr=rr, rw=rw, rr_any=bool(rr), P=sm.n_pairs)


def check_spec(spec, exp, what=""):
    """Every field of the parsed Spec against the restatement; the pair tables as sets, their indices a permutation of 0..P-1."""
    for k in ("S", "SB", "NQ", "J", "W", "NW", "qcol", "sh_begin", "jkind", "rr_any"):
        assert spec[k] == exp[k], (what, k, spec[k], exp[k])
    S, NW = exp["S"], exp["NW"]
    wl = spec["wl"] if NW > 0 else []
    wk = spec["wk"] if NW > 0 else []
    assert wl == exp["wl"] and wk == exp["wk"], (what, "wl/wk", spec["wl"], spec["wk"], exp["wl"], exp["wk"])
    rrp, wp = spec["rrp_"], spec["wp_"]
    assert len(rrp) == S * S and len(wp) == max(NW, 1) * S, (what, len(rrp), len(wp))
    rr = {(a, b) for a in range(S) for b in range(S) if rrp[a * S + b] >= 0}
    assert all(a < b for a, b in rr), (what, "a robot-robot pair stored at or below the diagonal", sorted(rr))
    assert rr == exp["rr"], (what, "robot-robot pairs", sorted(rr ^ exp["rr"]))
    rw = {(wl[i], a) for i in range(NW) for a in range(S) if wp[i * S + a] >= 0}
    assert rw == exp["rw"], (what, "robot-world pairs", sorted(rw ^ exp["rw"]))
    if NW == 0:
        assert all(v == -1 for v in wp), what
    idx = [v for v in rrp if v >= 0] + [v for v in wp if v >= 0]
    assert all(v == -1 for v in rrp + wp if v < 0), what
    assert sorted(idx) == list(range(exp["P"])), (what, "pair indices are not a permutation of 0..P-1", sorted(idx), exp["P"])


def with_unpaired_world_shape(sm, at=0):
    """``sm`` with one more world shape (a copy of its last one, moved far away) inserted at index ``at`` that has no pair: a
    descriptor with W = NW + 1, which Arm never produces (compile_scene lists a world shape with its first pair)."""
    S = sm.n_rshapes
    pose = sm.wshape_pose[-1].copy()
    pose[[3, 7, 11]] += 50.0
    pb = sm.pair_b.copy()
    pb[pb >= S + at] += 1
    return dataclasses.replace(
        sm, wshape_type=np.insert(sm.wshape_type, at, sm.wshape_type[-1]).astype(np.int32),
        wshape_pose=np.insert(sm.wshape_pose, at, pose, axis=0), wshape_param=np.insert(sm.wshape_param, at, sm.wshape_param[-1], axis=0),
        wshape_obj=np.insert(sm.wshape_obj, at, sm.wshape_obj[-1]).astype(np.int32), pair_b=pb.astype(np.int32))


def used_kernel(dev):
    return int(lib().nbk_broad_kernel_used(dev._h))


def assert_specialised(dev, what=""):
    used = used_kernel(dev)
    assert used == SPECIALISED, f"{what}: served by kernel {used}, not the specialised one"


# share of pairs, pooled over the generated cases, that are in contact in at least one of the first QUALITY_ROWS fuzz rows:
# 895 of 1304 when the case list was settled
QUALITY_ROWS = 3000
PAIR_SHARE = 0.68


def assert_input_quality(tmp):
    """Conditions on the fuzz inputs, computed with the float64 oracle alone.  At threshold 0 the colliding fraction of the fuzz
    batch lies in (0.002, 0.998) for at least three quarters of the generated robots (27 of 30 when the list was settled), and at
    least PAIR_SHARE (never below one half) of all their pairs touch in some row: a slot whose pair never collides cannot show a
    missed candidate."""
    from oracle.cpu_oracle import Oracle
    mixed = pairs = touching = 0
    for idx in range(len(SPEC_CASES)):
        arm, chain, obs = build_case(idx, tmp)
        orc = Oracle(arm.scene_model())
        q = sample(chain, FUZZ_B, 11)
        frac = float(orc.validity(q, 0.0, nthreads=8).mean())
        d = orc.proximity_jacobian(q[:QUALITY_ROWS])[0]
        hit = int((d <= 0).any(axis=0).sum())
        print(f"case {idx}: colliding fraction {frac:.4f}, pairs in contact {hit} of {d.shape[1]}")
        mixed += 0.002 < frac < 0.998
        pairs += d.shape[1]
        touching += hit
    print(f"{mixed} of {len(SPEC_CASES)} robots are neither always free nor always colliding; {touching} of {pairs} pairs touch somewhere")
    assert 4 * mixed >= 3 * len(SPEC_CASES), mixed
    assert PAIR_SHARE >= 0.5 and touching >= PAIR_SHARE * pairs, (touching, pairs)
