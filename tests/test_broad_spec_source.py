"""CPU tier of the per-robot broadphase tests: the ``struct Spec`` that ``bf32_spec_text`` (csrc/nbk_tables.hpp) generates for a robot against
an independent restatement from the scene model (spec_cases.expected_spec), over a fixed list of generated robots that spans the Spec
space; which robots get a source at all; and hipRTC compiling every one of them for gfx950.  No device is needed: the masks of the
same robots are tests/test_broad_spec.py."""
import dataclasses
import os
import time

import numpy as np
import pytest

import spec_cases as sc
from random_scenes import WORLD_KINDS
from spec_cases import SPEC_CASES


def _spec_of(sm):
    n, src = sc.spec_source(sm)
    assert n > 0, "no source for an eligible robot"
    return sc.parse_spec(src), src


@pytest.fixture(scope="module")
def sources(tmp_path_factory):
    """{case: (parsed Spec, restated Spec, source, URDF text or None)} of every generated and named case."""
    tmp = str(tmp_path_factory.mktemp("spec_source"))
    out = {}
    for key in list(range(len(SPEC_CASES))) + list(sc.NAMED_CASES):
        arm, chain, obs = sc.any_case(key, tmp)
        sm = arm.scene_model()
        spec, src = _spec_of(sm)
        urdf = open(os.path.join(tmp, f"spec_case_{key}.urdf")).read() if isinstance(key, int) else None
        out[key] = (spec, sc.expected_spec(sm), src, urdf)
    return out


def test_spec_equals_the_scene_model(sources):
    """Every table of the generated Spec, for 30 generated robots and c2 / c2m / plane_hull: sizes, q columns, shapes per frame,
    joint kinds, the world shapes with a pair and their kinds, and both pair tables as sets with their indices a permutation of
    0..P-1.  The generated cases also against what the generator was asked for."""
    for key, (spec, exp, src, urdf) in sources.items():
        sc.check_spec(spec, exp, key)
        if isinstance(key, int):
            n_joints, n_shapes, mode, base, fixed, kinds = SPEC_CASES[key]
            assert (spec["J"], spec["S"]) == (n_joints, n_shapes), key
            assert (spec["sh_begin"][1] > 0) == base, key
            # joint kinds from the URDF text itself: prismatic -> 4; an axis written as +-1 on one coordinate -> that coordinate
            want = []
            for joint in urdf.split("<joint ")[1:]:
                if 'type="fixed"' in joint:
                    continue
                ax = [float(v) for v in joint.split('<axis xyz="')[1].split('"')[0].split()]
                unit = [e for e in range(3) if abs(ax[e]) == 1.0 and ax[(e + 1) % 3] == 0.0 and ax[(e + 2) % 3] == 0.0]
                want.append(4 if 'type="prismatic"' in joint else (unit[0] if unit else 3))
            assert spec["jkind"] == want, (key, spec["jkind"], want)
            assert spec["wk"][:spec["NW"]] == [sc.CORE_KIND[WORLD_KINDS.index(k)] for k in kinds], key
            # Arm lists a world shape with its first pair: the third obstacle of the removal cases, all pairs removed, is not in the model
            assert spec["W"] == spec["NW"] == len(kinds), key


def test_case_list_spans_the_spec_space(sources):
    """The coverage the case list exists for; a change of the generator or the list that loses one of these fails here."""
    gen = [sources[k][0] for k in range(len(SPEC_CASES))]
    assert {s["S"] for s in gen} >= {1, 2, 7, 8, 9, 12, 13, 15, 16}
    assert {s["SB"] for s in gen} == {8, 12, 16}
    assert {s["J"] for s in gen} >= {1, 2, 7, 8}
    assert {k for s in gen for k in s["jkind"]} == {0, 1, 2, 3, 4}
    assert {s["NW"] for s in gen} == {0, 1, 2}
    assert {s["wk"][0] for s in gen if s["NW"] >= 1} == {0, 1, 2, 3, 4, 5}
    assert {s["wk"][1] for s in gen if s["NW"] == 2} == {0, 1, 2, 3, 4, 5}
    assert any(not s["rr_any"] for s in gen) and any(s["rr_any"] for s in gen)
    assert any(s["sh_begin"][1] > 0 for s in gen) and any(s["sh_begin"][1] == 0 for s in gen)
    # frames without shapes, frames with two or three, odd S, S < SB
    assert any(0 in np.diff(s["sh_begin"][1:]) for s in gen) and any(3 in np.diff(s["sh_begin"]) for s in gen)
    assert any(s["S"] % 2 == 1 for s in gen) and any(s["S"] < s["SB"] for s in gen)
    # removals: at least a third of the robots; among them slot groups (2i, 2i + 1) of a robot-robot row and of a world row with
    # exactly one pair, and a robot-robot row with none while later rows have some
    removed = [k for k in range(len(SPEC_CASES)) if sc.has_removals(k)]
    assert 3 * len(removed) >= len(SPEC_CASES)
    half_rr = half_w = empty_row = False
    for k in removed:
        s = sources[k][0]
        S = s["S"]
        rr = lambda a, b: a < b < S and s["rrp_"][a * S + b] >= 0
        wp = lambda i, a: a < S and s["wp_"][i * S + a] >= 0
        for a in range(S):
            half_rr = half_rr or any(rr(a, 2 * i) != rr(a, 2 * i + 1) and 2 * i > a for i in range(8))
            empty_row = empty_row or (a < S - 2 and not any(rr(a, b) for b in range(S)) and any(rr(c, b) for c in range(a + 1, S) for b in range(S)))
        for i in range(s["NW"]):
            half_w = half_w or any(wp(i, 2 * g) != wp(i, 2 * g + 1) for g in range(8))
    assert half_rr and half_w and empty_row
    # at most a third of the robots carry hulls (they are the slow ones)
    assert 3 * sum("mesh" in c[5] for c in SPEC_CASES) <= len(SPEC_CASES)


def test_unpaired_world_shape_keeps_its_slot(tmp_path):
    """W = 3, NW = 2: a world shape without a pair ahead of the two that have some, so that ``wl`` is (1, 2) and not 0..NW-1 and
    ``wk`` must be read through it.  The Arm API cannot produce this descriptor (see build_case); the library accepts it."""
    arm, chain, obs = sc.build_case(sc.EDGE_CASE, str(tmp_path))
    sm = arm.scene_model()
    assert sm.wshape_type[0] != sm.wshape_type[1]
    for at in (0, 1, 2):
        sm3 = sc.with_unpaired_world_shape(sm, at)
        spec, src = _spec_of(sm3)
        exp = sc.expected_spec(sm3)
        assert (exp["W"], exp["NW"]) == (3, 2) and exp["wl"] == [w for w in range(3) if w != at]
        sc.check_spec(spec, exp, at)
    # three world shapes with pairs: no source
    sm4 = dataclasses.replace(sc.with_unpaired_world_shape(sm, 0))
    sm4.pair_b = sm4.pair_b.copy()
    sm4.pair_b[np.flatnonzero(sm4.pair_b >= sm4.n_rshapes)[0]] = sm4.n_rshapes        # its first world pair now names shape 0
    assert sc.expected_spec(sm4)["NW"] == 3 and sc.spec_source(sm4)[0] == 0


def test_q_columns_follow_the_model_when_nq_exceeds_j(tmp_path):
    """NQ > J and a permuted q layout: URDF chains always have NQ = J, the KinematicModel arrays can say otherwise."""
    arm, chain, obs = sc.build_case(5, str(tmp_path))
    sm = arm.scene_model()
    J = sm.kin.n_joints
    qidx = np.random.default_rng(5).permutation(J + 2)[:J].astype(np.int32)
    sm2 = dataclasses.replace(sm, kin=dataclasses.replace(sm.kin, n_q=J + 2, joint_qidx=qidx))
    spec, src = _spec_of(sm2)
    assert spec["NQ"] == J + 2 and spec["qcol"] == qidx.tolist()
    sc.check_spec(spec, sc.expected_spec(sm2))
    assert sc.lib().nbk_jit_compile(src, b"gfx950") > 0, sc.lib().nbk_last_error()


def _robot(tmp, name, **kw):
    from numbotics_amd.physics import GraphChain
    from numbotics_amd.robots import Arm
    from random_scenes import random_spec_robot
    sc.fresh()
    rng = np.random.default_rng(77)
    chain = GraphChain.from_urdf(random_spec_robot(rng, os.path.join(tmp, name + ".urdf"), **kw))
    return Arm(chain), chain, rng


def _has_source(arm):
    return sc.spec_source(arm.scene_model())[0] > 0


def test_eight_joints_are_served_nine_are_not(tmp_path):
    arm, chain, rng = _robot(str(tmp_path), "j8", n_joints=8, n_shapes=9, axis_mode="mixed")
    assert chain.dof == 8 and _has_source(arm)
    arm, chain, rng = _robot(str(tmp_path), "j9", n_joints=9, n_shapes=9, axis_mode="mixed")
    assert chain.dof == 9 and arm.scene_model().n_pairs > 0 and not _has_source(arm)


def test_sixteen_shapes_are_served_seventeen_are_not(tmp_path):
    arm, chain, rng = _robot(str(tmp_path), "s16", n_joints=8, n_shapes=16, axis_mode="aligned")
    assert arm.scene_model().n_rshapes == 16 and _has_source(arm)
    arm, chain, rng = _robot(str(tmp_path), "s17", n_joints=8, n_shapes=17, axis_mode="aligned")
    assert arm.scene_model().n_rshapes == 17 and not _has_source(arm)


def test_two_world_shapes_are_served_three_are_not(tmp_path):
    from random_scenes import spec_obstacles
    arm, chain, rng = _robot(str(tmp_path), "w", n_joints=4, n_shapes=5, axis_mode="mixed")
    obs = spec_obstacles(rng, ("box", "sphere"), 0.5)
    assert arm.scene_model().n_wshapes == 2 and _has_source(arm)
    obs += spec_obstacles(rng, ("capsule",), 0.5, first=2)
    assert arm.scene_model().n_wshapes == 3 and not _has_source(arm)
    # with the third one's pairs removed the scene is served again
    for link in chain._links:
        arm.remove_collision_pair(link, obs[2])
    assert arm.scene_model().n_wshapes == 2 and _has_source(arm)


def test_a_branching_tree_is_not_served(tmp_path):
    from numbotics_amd.physics import GraphChain
    from numbotics_amd.robots import Arm
    from random_scenes import spec_obstacles
    ball = '<collision><origin xyz="0.03 0 0" rpy="0 0 0"/><geometry><sphere radius="0.04"/></geometry></collision>'
    joint = ('<joint name="j{c}" type="revolute"><origin xyz="{x} 0 0.1" rpy="0 0 0"/><parent link="l{p}"/><child link="l{c}"/>'
             '<axis xyz="0 0 1"/><limit lower="-2" upper="2" effort="1" velocity="1"/></joint>')
    for name, parents in (("serial", (0, 1, 2)), ("tree", (0, 1, 1))):
        text = ['<?xml version="1.0"?>', '<robot name="t">'] + [f'<link name="l{i}">{ball}</link>' for i in range(4)]
        text += [joint.format(c=c + 1, p=p, x=0.1 * (c - 1)) for c, p in enumerate(parents)] + ["</robot>"]
        path = os.path.join(str(tmp_path), name + ".urdf")
        with open(path, "w") as f:
            f.write("\n".join(text))
        sc.fresh()
        arm = Arm(GraphChain.from_urdf(path))
        obs = spec_obstacles(np.random.default_rng(1), ("box",), 0.4)
        assert arm.scene_model().n_pairs > 0
        assert _has_source(arm) == (name == "serial"), name


def test_a_scene_without_a_pair_is_not_served(tmp_path):
    arm, chain, rng = _robot(str(tmp_path), "nopair", n_joints=1, n_shapes=2, axis_mode="random", base_shapes=True)
    sm = arm.scene_model()
    assert sm.n_rshapes == 2 and sm.n_pairs == 0 and sc.spec_source(sm)[0] == 0


def test_trailing_fixed_joints_are_served(tmp_path):
    arm, chain, rng = _robot(str(tmp_path), "trail", n_joints=3, n_shapes=6, axis_mode="mixed", fixed_joints=2)
    text = open(os.path.join(str(tmp_path), "trail.urdf")).read()
    assert text.rstrip().split("<joint ")[-1].startswith('name="j5" type="fixed"')
    sm = arm.scene_model()
    assert sm.kin.n_joints == 3 and chain.dof == 3 and _has_source(arm)
    sc.check_spec(_spec_of(sm)[0], sc.expected_spec(sm))


def test_every_eligible_source_compiles_for_gfx950(sources):
    """hipRTC takes every generated source (all 33: none is left out), which also checks the static_assert on the LDS queue room
    in nbk_bf32_spec.hpp for every (NQ, SB) of the list."""
    L = sc.lib()
    t0 = time.time()
    for key, (spec, exp, src, urdf) in sources.items():          # one after the other: hipRTC compiles one program at a time
        t1 = time.time()
        size = L.nbk_jit_compile(src, b"gfx950")
        assert size > 0, (key, L.nbk_last_error())
        print(f"case {key}: S={spec['S']} J={spec['J']} NW={spec['NW']} P={exp['P']}: {size} bytes in {time.time() - t1:.2f} s")
    print(f"compile sweep: {time.time() - t0:.1f} s")


def test_fuzz_inputs_are_not_trivial(tmp_path):
    """The input-quality conditions of the GPU fuzz (test_broad_spec.py), which need the oracle only: see spec_cases.assert_input_quality."""
    sc.assert_input_quality(str(tmp_path))
