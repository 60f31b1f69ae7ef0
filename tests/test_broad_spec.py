"""The float32 broadphase compiled per robot (numbotics_amd/csrc/nbk_bf32_spec.hpp): its masks against the generic kernel's
(NBK_NO_JIT=1 in a child process) and the oracle, rebuilds after pair / world changes, the fall-back when hipRTC fails, graph
replay.  The first test needs no GPU: it compiles the generated source for gfx950 with hipRTC.  The second half runs the robots of
spec_cases.py (whose generated tables test_broad_spec_source.py checks on the CPU) and the input edges -- tail waves, misaligned
slabs, extreme thresholds, non-finite rows, waves with one wide lane, queue overflow, tiles, streams -- through the specialised
kernel; every assertion there comes after the check that this kernel, and not the generic one, served the call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import spec_cases as sc
from numbotics_amd.scenes import build_scene, sample_q

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
THRESHOLDS = (0.0, 1e-6, 0.01, -0.002)
B = 1 << 16
GENERIC, SPECIALISED = 1, 2


_lib = sc.lib
_fresh = sc.fresh
_spec_source = sc.spec_source


def test_generated_source_compiles_for_gfx950():
    """CPU only: the spec generator's output for the headline robot compiles with hipRTC; a bad target is an error, not a crash."""
    _fresh()
    arm, chain, obs = build_scene("c2")
    n, src = _spec_source(arm.scene_model())
    assert n > 0 and b"struct Spec" in src and b"k_broad_f32_spec" in src
    lib = _lib()
    assert lib.nbk_jit_compile(src, b"gfx950") > 0, lib.nbk_last_error()
    assert lib.nbk_jit_compile(src, b"gfx000") < 0
    assert lib.nbk_jit_compile(src + b"\nthis is not C++;\n", b"gfx950") < 0      # the compiler's own error path
    assert b"failed" in lib.nbk_last_error()
    # robots the kernel does not serve get no source: a scene with more world shapes than the kernel unrolls (8 cubes)
    _fresh()
    arm3, chain3, obs3 = build_scene("c3")
    assert _spec_source(arm3.scene_model())[0] == 0


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

def _random_arm(tmp):
    from numbotics_amd.physics import GraphChain
    from numbotics_amd.robots import Arm
    from random_scenes import random_urdf, random_obstacles
    rng = np.random.default_rng(7)
    chain = GraphChain.from_urdf(random_urdf(rng, 7, os.path.join(tmp, "spec_random.urdf"), max_back=1))
    arm = Arm(chain)
    obs = random_obstacles(rng, 1)
    return arm, chain, obs


def _case(name, tmp):
    """-> (arm, chain, obstacles) of one named case; built the same way in the parent and in the child process."""
    if name == "c2_wide":
        return build_scene("c2")
    if name == "random":
        return _random_arm(tmp)
    if name in ("plane_hull", "plane_hull_wide"):
        # at most 2 world shapes, neither a box: the plane and hull branches of both stages
        from numbotics_amd.physics import GraphChain, Mesh, Plane
        from numbotics_amd.robots import Arm
        from numbotics_amd.scenes import KINOVA_URDF, MESH_DIR, apply_rrt_script_removals
        chain = GraphChain.from_urdf(KINOVA_URDF)
        arm = Arm(chain)
        apply_rrt_script_removals(arm)
        obs = [Plane(0.0, np.array([0.0, 0.0, 1.0]), position=np.array([0.0, 0.0, -0.3])),
               Mesh(0.0, os.path.join(MESH_DIR, "rock.obj"), position=np.array([0.55, 0.25, 0.45]))]
        return arm, chain, obs
    if name == "c2_removed":
        arm, chain, obs = build_scene("c2")
        arm.remove_collision_pair("base_link", "forearm_link")
        arm.remove_collision_pair("shoulder_link", "bracelet_link")
        return arm, chain, obs
    return build_scene(name)


CASES = ("c2", "c3", "c2m", "c5m", "random", "c2_removed", "plane_hull", "plane_hull_wide", "c2_wide")
# the specialised kernel must have served these
SPECIALISED_CASES = ("c2", "c2m", "c2_removed", "random", "plane_hull", "plane_hull_wide", "c2_wide")


def _sample(chain, n, seed, name=""):
    """Uniform over the joint limits; continuous joints over [-pi, pi].  "*_wide" cases: every joint value moved by +-4 pi (the
    same poses up to rounding), so that every lane's |q| sum exceeds the 64 rad the fast stage's static slack covers and the
    kernel takes its general stage."""
    lim = np.asarray(chain.joint_limits, dtype=np.float64)
    lim = np.where(np.isfinite(lim), lim, np.sign(lim) * np.pi)
    q = np.random.default_rng(seed).uniform(lim[:, 0], lim[:, 1], (n, chain.dof))
    if name.endswith("_wide"):
        q = q + np.where(np.arange(n)[:, None] % 2 == 0, 4.0, -4.0) * np.pi
    return q


def _masks(names, tmp):
    out = {}
    for name in names:
        _fresh()
        arm, chain, obs = _case(name, tmp)
        q = _sample(chain, B, 11, name)
        for thr in THRESHOLDS:
            out[f"{name}|{thr}"] = arm.in_collision(q, thr)
        out[f"{name}|used"] = np.int32(_lib().nbk_broad_kernel_used(arm._scene_device()[1]._h))
    return out


def _child_masks(tmp, env_extra):
    """The masks of every case in a fresh process with `env_extra` set."""
    out = os.path.join(tmp, "child_masks.npz")
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {HERE!r}); import numpy as np; import test_broad_spec as t; "
            f"np.savez({out!r}, **{{k.replace('|', '@'): v for k, v in t._masks({list(CASES)!r}, {tmp!r}).items()}})")
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(out) as z:
        return {k.replace("@", "|"): z[k] for k in z.files}


@pytest.mark.gpu
def test_specialised_masks_equal_generic_and_oracle(tmp_path):
    from oracle.cpu_oracle import Oracle
    tmp = str(tmp_path)
    generic = _child_masks(tmp, {"NBK_NO_JIT": "1"})
    mine = _masks(CASES, tmp)
    for name in CASES:
        assert int(generic[f"{name}|used"]) == GENERIC, name
        for thr in THRESHOLDS:
            assert np.array_equal(mine[f"{name}|{thr}"], generic[f"{name}|{thr}"]), f"{name} at {thr}: specialised != generic"
    # the serial-chain cases with few world shapes ran the specialised kernel
    for name in SPECIALISED_CASES:
        assert int(mine[f"{name}|used"]) == SPECIALISED, name
    # and the oracle agrees (every threshold)
    for name in ("c2", "c2_removed", "plane_hull", "plane_hull_wide", "c2_wide"):
        _fresh()
        arm, chain, obs = _case(name, tmp)
        q = _sample(chain, B, 11, name)
        orc = Oracle(arm.scene_model())
        for thr in THRESHOLDS:
            assert np.array_equal(mine[f"{name}|{thr}"], orc.validity(q, thr, nthreads=8)), f"{name} at {thr}: != oracle"


@pytest.mark.gpu
def test_instance_follows_pair_and_world_changes():
    """remove_collision_pair and a new obstacle give a new descriptor with its own specialised kernel; masks stay the oracle's."""
    from oracle.cpu_oracle import Oracle
    from numbotics_amd.physics import Cube
    lib = _lib()
    _fresh()
    arm, chain, obs = build_scene("c2")
    q = sample_q(chain, B, seed=3)
    arm.in_collision(q)
    h0 = arm._scene_device()[1]._h.value
    assert lib.nbk_broad_kernel_used(arm._scene_device()[1]._h) == SPECIALISED
    src0 = _spec_source(arm.scene_model())[1]
    arm.remove_collision_pair("base_link", "forearm_link")
    src1 = _spec_source(arm.scene_model())[1]
    assert src1 != src0
    m = arm.in_collision(q)
    assert arm._scene_device()[1]._h.value != h0
    assert lib.nbk_broad_kernel_used(arm._scene_device()[1]._h) == SPECIALISED
    assert np.array_equal(m, Oracle(arm.scene_model()).validity(q, nthreads=8))
    obs.append(Cube(half_extent=0.1, mass=0.0, position=np.array([0.0, 0.5, 0.5])))
    src2 = _spec_source(arm.scene_model())[1]
    assert src2 != src1
    m = arm.in_collision(q)
    assert lib.nbk_broad_kernel_used(arm._scene_device()[1]._h) == SPECIALISED
    assert np.array_equal(m, Oracle(arm.scene_model()).validity(q, nthreads=8))
    # small calls never compile: a fresh descriptor's first call below 2^16 configurations takes the generic kernel
    _fresh()
    arm2, chain2, obs2 = build_scene("c2")
    arm2.in_collision(q[:4096])
    assert lib.nbk_broad_kernel_used(arm2._scene_device()[1]._h) in (0, GENERIC, 3)


@pytest.mark.gpu
def test_compile_failure_falls_back(tmp_path):
    """A failed compile keeps the generic kernel and the same masks: a source hipRTC rejects (NBK_JIT_OPTIONS makes the launch
    bound an undeclared name, so the compiler itself reports the error) and a target the library refuses before calling hipRTC (NBK_JIT_ARCH)."""
    tmp = str(tmp_path)
    mine = _masks(("c2",), tmp)
    assert int(mine["c2|used"]) == SPECIALISED
    for env in ({"NBK_JIT_OPTIONS": "-DNBK_SPEC_WAVES=no_such_name"}, {"NBK_JIT_ARCH": "gfx000"}):
        bad = _child_masks(tmp, env)
        assert int(bad["c2|used"]) == GENERIC, env
        for thr in THRESHOLDS:
            assert np.array_equal(bad[f"c2|{thr}"], mine[f"c2|{thr}"]), env


@pytest.mark.gpu
def test_graph_replays_specialised_launch():
    import torch
    lib = _lib()
    _fresh()
    arm, chain, obs = build_scene("c2")
    _, dev = arm._scene_device()
    q = torch.from_numpy(sample_q(chain, B, seed=21)).cuda()
    words = torch.zeros(((B + 63) // 64,), dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        st = C.c_void_p(side.cuda_stream)
        assert lib.nbk_validity_batch(dev._h, q.data_ptr(), B, 0.0, words.data_ptr(), None, st) == 0    # compiles, allocates
        side.synchronize()
        assert lib.nbk_broad_kernel_used(dev._h) == SPECIALISED
        g = torch.cuda.CUDAGraph()
        g.capture_begin()
        assert lib.nbk_validity_batch(dev._h, q.data_ptr(), B, 0.0, words.data_ptr(), None, st) == 0
        g.capture_end()
    torch.cuda.current_stream().wait_stream(side)
    assert lib.nbk_broad_kernel_used(dev._h) == SPECIALISED
    for seed in (22, 23):
        q.copy_(torch.from_numpy(sample_q(chain, B, seed=seed)).cuda())
        words.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(words.cpu().numpy(), dev.validity(q, 0.0, packed=True).cpu().numpy())


# ---- the Spec space and the input edges, on the specialised kernel -------------------------------------------------------------

def _validity(dev, q, thr, what, **kw):
    """One validity call that must have been served by the specialised kernel."""
    out = dev.validity(q, thr, **kw)
    sc.assert_specialised(dev, what)
    return out


def _fuzz_masks(keys, tmp):
    """{"<case>|<thr>": packed mask bits, "<case>|used": kernel} of the fuzz batch of every generated case in ``keys``."""
    out = {}
    for key in keys:
        arm, chain, obs = sc.build_case(key, tmp)
        _, dev = arm._scene_device()
        q = sc.sample(chain, sc.FUZZ_B, 11)
        used = set()
        for thr in sc.THRESHOLDS:
            out[f"{key}|{thr}"] = np.packbits(dev.validity(q, thr))
            used.add(sc.used_kernel(dev))
        out[f"{key}|used"] = np.array(sorted(used), dtype=np.int32)
    return out


def _child_fuzz_masks(tmp):
    """The fuzz masks of every generated case from the generic kernel: ONE fresh process with NBK_NO_JIT=1."""
    out = os.path.join(tmp, "child_fuzz_masks.npz")
    keys = list(range(len(sc.SPEC_CASES)))
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {HERE!r}); import numpy as np; import test_broad_spec as t; "
            f"np.savez({out!r}, **{{k.replace('|', '@'): v for k, v in t._fuzz_masks({keys!r}, {tmp!r}).items()}})")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, NBK_NO_JIT="1"), cwd=ROOT, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(out) as z:
        return {k.replace("@", "|"): z[k] for k in z.files}


def _report(name, thr, q, orc, spec, ref, generic=None):
    """Which rows differ, who disagrees with whom, and the oracle's closest pair there (the style of tools/mismatch.py)."""
    rows = np.flatnonzero(spec != ref)
    lines = [f"case {name} at threshold {thr}: {rows.size} rows differ from the oracle (first: {rows[:8].tolist()})"]
    for b in rows[:4]:
        d = orc.proximity_jacobian(q[b:b + 1])[0][0]
        g = "" if generic is None else f" generic={bool(generic[b])}"
        lines.append(f"  row {b}: oracle={bool(ref[b])} spec={bool(spec[b])}{g}; closest pair {int(np.argmin(d))} at {d.min():.3e}; q={q[b].tolist()}")
    return "\n".join(lines)


@pytest.mark.gpu
def test_spec_space_fuzz(tmp_path):
    """The 30 generated robots of spec_cases.SPEC_CASES (S 1-16, J 1-8, every joint kind, 0-2 world shapes of every kind, pair
    removals, shapes on the base or not; sharp and Bullet-margin shapes alternating), 2^16 + 37 rows uniform over the limits, four
    thresholds: the specialised kernel's masks equal the float64 oracle's bit for bit, and the generic kernel's (second witness).
    The inputs are not trivial: 27 of the 30 robots have a colliding fraction strictly between 0.002 and 0.998 at threshold 0 (at
    least three quarters are required), and 895 of their 1304 pairs (0.686; at least spec_cases.PAIR_SHARE = 0.68 >= 1/2 is required)
    are in contact in one of the first 3000 rows, both computed with the oracle alone."""
    from oracle.cpu_oracle import Oracle
    tmp = str(tmp_path)
    sc.assert_input_quality(tmp)
    generic = _child_fuzz_masks(tmp)
    for key in range(len(sc.SPEC_CASES)):
        assert generic[f"{key}|used"].tolist() == [sc.GENERIC], key
        arm, chain, obs = sc.build_case(key, tmp)
        sm, dev = arm._scene_device()
        orc = Oracle(sm)
        q = sc.sample(chain, sc.FUZZ_B, 11)
        for thr in sc.THRESHOLDS:
            mine = _validity(dev, q, thr, f"case {key} at {thr}")
            ref = orc.validity(q, thr, nthreads=8)
            gen = np.unpackbits(generic[f"{key}|{thr}"])[:sc.FUZZ_B].astype(bool)
            assert np.array_equal(mine, ref), _report(key, thr, q, orc, mine, ref, gen)
            assert np.array_equal(mine, gen), f"case {key} at {thr}: specialised != generic in rows {np.flatnonzero(mine != gen)[:8].tolist()}"
        print(f"case {key}: {sc.SPEC_CASES[key]} served by kernel {sc.used_kernel(dev)}, {int(ref.sum())} of {sc.FUZZ_B} collide at {thr}")


EDGE_SCENES = ("c2", "plane_hull", sc.EDGE_CASE)


def _edge_scene(key, tmp):
    from oracle.cpu_oracle import Oracle
    arm, chain, obs = sc.any_case(key, tmp)
    sm, dev = arm._scene_device()
    return arm, chain, obs, sm, dev, Oracle(sm)


@pytest.mark.gpu
@pytest.mark.parametrize("key", EDGE_SCENES, ids=str)
def test_spec_tail_waves_views_and_thresholds(key, tmp_path):
    """Batch sizes 2^16 + {0, 1, 63, 64, 65} as bytes and as packed words (unused bits of the last word zero); device views that
    start at rows 1 and 3 of a larger tensor -- with an odd NQ the slab is 8- but not 16-byte aligned (the scalar copy branch), with
    an even NQ it stays 16-byte aligned (the double2 branch) and the batch ends in a tail wave either way; thresholds at which
    everything / nothing collides.  A NaN threshold is not tried: the oracle does not define one."""
    import torch
    from numbotics_amd.parallel import unpack_mask
    arm, chain, obs, sm, dev, orc = _edge_scene(key, str(tmp_path))
    n_q = sm.kin.n_q
    B0 = sc.SPEC_MIN_BATCH
    q = sc.sample(chain, B0 + 65 + 4, 31)
    ref = orc.validity(q, 0.0, nthreads=8)
    qt = torch.from_numpy(q).cuda()
    for r in (0, 1, 63, 64, 65):
        B = B0 + r
        got = _validity(dev, qt[:B], 0.0, f"{key} B={B}")
        assert np.array_equal(got.cpu().numpy(), ref[:B]), (key, B, np.flatnonzero(got.cpu().numpy() != ref[:B])[:8])
        words = _validity(dev, qt[:B], 0.0, f"{key} B={B} packed", packed=True).cpu().numpy()
        assert words.shape == ((B + 63) // 64,) and np.array_equal(unpack_mask(words, B), ref[:B]), (key, B, "packed")
        if B % 64:
            assert int(words.view(np.uint64)[-1]) >> (B % 64) == 0, (key, B, "bits beyond B in the last word")
    for lo in (1, 3):
        view = qt[lo:lo + B0 + 37]
        assert view.is_contiguous() and view.data_ptr() % 16 == (8 if n_q % 2 else 0), (key, lo)
        got = _validity(dev, view, 0.0, f"{key} view at row {lo}")
        assert np.array_equal(got.cpu().numpy(), ref[lo:lo + B0 + 37]), (key, lo)
        words = _validity(dev, view, 0.0, f"{key} view at row {lo} packed", packed=True).cpu().numpy()
        assert np.array_equal(unpack_mask(words, B0 + 37), ref[lo:lo + B0 + 37]), (key, lo, "packed")
    for thr in (1e6, -1e6, 5.0, -5.0):
        want = orc.validity(q[:B0 + 37], thr, nthreads=8)
        assert want.all() if thr > 0 else not want.any()
        assert np.array_equal(_validity(dev, q[:B0 + 37], thr, f"{key} at {thr}"), want), (key, thr)
    print(f"{key}: tail waves, views and extreme thresholds served by kernel {sc.used_kernel(dev)}; {int(ref.sum())} of {ref.size} collide")


def _moved(sm, q, rows, rng):
    """``q`` with the rows ``rows`` sent far outside the limits: revolute columns by +-4 pi k (k up to 500, the same pose up to
    rounding), prismatic columns times 40."""
    q = q.copy()
    kin = sm.kin
    for k in range(kin.n_joints):
        col = int(kin.joint_qidx[k])
        if kin.joint_type[k] == 1:
            q[rows, col] *= 40.0
        else:
            q[rows, col] += 4.0 * np.pi * rng.integers(1, 501, rows.size) * rng.choice([-1.0, 1.0], rows.size)
    return q


@pytest.mark.gpu
@pytest.mark.parametrize("key", EDGE_SCENES, ids=str)
def test_spec_waves_with_one_bad_or_wide_lane(key, tmp_path):
    """The stage is chosen per wave, so one lane decides for 64.  Non-finite rows: nan / +inf / -inf in one column of 300 random
    rows of 2^16 + 37, more than half of them the only bad lane of their wave -- they collide, all others equal the oracle.  Mixed waves: one row of
    every 64, and separately one of every 997, far outside the limits (see _moved) while its neighbours stay inside: the moved rows
    and their neighbours, which the wide lane takes through the general stage with it, all equal the oracle."""
    arm, chain, obs, sm, dev, orc = _edge_scene(key, str(tmp_path))
    B = sc.SPEC_MIN_BATCH + 37
    q = sc.sample(chain, B, 41)
    rng = np.random.default_rng(42)
    bad = q.copy()
    bad_rows = rng.choice(B, 300, replace=False)
    bad[bad_rows, rng.integers(0, sm.kin.n_q, 300)] = rng.choice([np.nan, np.inf, -np.inf], 300)
    per_wave = np.bincount(bad_rows // 64)
    assert per_wave.max() < 32 and 2 * int((per_wave == 1).sum()) >= 300           # most bad lanes are the only one of their wave
    ref = orc.validity(bad, 0.0, nthreads=8)
    got = _validity(dev, bad, 0.0, f"{key} non-finite")
    assert ref[bad_rows].all() and got[bad_rows].all(), key
    assert np.array_equal(got, ref), (key, "non-finite", np.flatnonzero(got != ref)[:8])
    for step, first in ((64, 17), (997, 5)):
        rows = np.arange(first, B, step)
        wide = _moved(sm, q, rows, rng)
        others = np.setdiff1d(np.arange(B), rows)
        assert np.array_equal(wide[others], q[others])
        for thr in (0.0, 0.01):
            ref = orc.validity(wide, thr, nthreads=8)
            got = _validity(dev, wide, thr, f"{key} every {step}th row wide")
            assert np.array_equal(got[rows], ref[rows]), (key, step, thr, "moved rows", rows[got[rows] != ref[rows]][:8])
            assert np.array_equal(got[others], ref[others]), (key, step, thr, "neighbours", others[got[others] != ref[others]][:8])
            # the neighbours' verdicts are those of the same rows in a batch without a wide lane
            assert np.array_equal(got[others], orc.validity(q, thr, nthreads=8)[others]), (key, step, thr)
            print(f"{key}: every {step}th row wide at {thr} served by kernel {sc.used_kernel(dev)}; {int(ref[rows].sum())} of {rows.size} moved rows collide")


@pytest.mark.gpu
@pytest.mark.parametrize("key", EDGE_SCENES, ids=str)
def test_generic_waves_with_one_wide_lane(key, tmp_path):
    """The generic k_broad_f32 (a batch below SPEC_MIN_BATCH) through its general stage against plane, box and hull world shapes:
    row 17 of every wave of 4096 + 37 rows is far outside the limits (see _moved) and takes its 63 neighbours through the general
    stage with it.  The moved rows and the neighbours equal the oracle, and the neighbours equal the oracle's verdicts of the batch
    without a wide lane.  Not trivial, by the oracle alone: at least 5 of the 65 moved rows collide and at least 5 are free, and
    between 5 % and 95 % of the neighbours collide."""
    arm, chain, obs, sm, dev, orc = _edge_scene(key, str(tmp_path))
    B = 4096 + 37
    assert B < sc.SPEC_MIN_BATCH
    q = sc.sample(chain, B, 41)
    rows = np.arange(17, B, 64)
    wide = _moved(sm, q, rows, np.random.default_rng(42))
    others = np.setdiff1d(np.arange(B), rows)
    assert rows.size == 65 and np.array_equal(wide[others], q[others])
    for thr in (0.0, 0.01):
        ref = orc.validity(wide, thr, nthreads=8)
        plain = orc.validity(q, thr, nthreads=8)
        print(f"{key} at {thr}: {int(ref[rows].sum())} of {rows.size} moved rows collide, {ref[others].mean():.3f} of the others")
        assert 5 <= int(ref[rows].sum()) <= rows.size - 5, (key, thr, int(ref[rows].sum()))
        assert 0.05 <= ref[others].mean() <= 0.95, (key, thr, ref[others].mean())
        got = dev.validity(wide, thr)
        assert sc.used_kernel(dev) == sc.GENERIC, (key, thr, sc.used_kernel(dev))
        assert np.array_equal(got[rows], ref[rows]), (key, thr, "moved rows", rows[got[rows] != ref[rows]][:8])
        assert np.array_equal(got[others], ref[others]), (key, thr, "neighbours", others[got[others] != ref[others]][:8])
        assert np.array_equal(got[others], plain[others]), (key, thr, "neighbours against the batch without a wide lane")


@pytest.mark.gpu
@pytest.mark.parametrize("key", ("c2", sc.EDGE_CASE), ids=str)
def test_spec_queue_overflow_is_redecided(key, tmp_path):
    """The item queue shrunk to a few KB (as test_queue_overflow_is_redecided_without_a_queue does for the generic kernel): blocks
    of the specialised kernel that overflow mark themselves and are decided again without a queue.  Both workspaces, bytes and
    packed words, and the default budget afterwards."""
    import torch
    from numbotics_amd._lib import debug_option
    from numbotics_amd.parallel import unpack_mask
    arm, chain, obs, sm, dev, orc = _edge_scene(key, str(tmp_path))
    B = sc.SPEC_MIN_BATCH + 37
    q = sc.sample(chain, B, 51)
    refs = {thr: orc.validity(q, thr, nthreads=8) for thr in (0.0, 0.02)}
    for budget in (1 << 12, 1 << 17, 1 << 21):
        with debug_option("queue_budget", budget):
            for thr, ref in refs.items():
                assert np.array_equal(_validity(dev, q, thr, f"{key} budget {budget}"), ref), (key, budget, thr)
                words = _validity(dev, q, thr, f"{key} budget {budget} packed", packed=True)
                assert np.array_equal(unpack_mask(words, B), ref), (key, budget, thr, "packed")
            ws = torch.empty((dev.validity_workspace_bytes(B),), dtype=torch.uint8, device="cuda")
            for thr, ref in refs.items():
                assert np.array_equal(_validity(dev, q, thr, f"{key} budget {budget} caller workspace", workspace=ws), ref), (key, budget, thr)
                words = _validity(dev, q, thr, f"{key} budget {budget} caller workspace packed", packed=True, workspace=ws)
                assert np.array_equal(unpack_mask(words, B), ref), (key, budget, thr, "caller workspace, packed")
    assert np.array_equal(_validity(dev, q, 0.0, f"{key} default budget"), refs[0.0])
    print(f"{key}: queue budgets served by kernel {sc.used_kernel(dev)}; {int(refs[0.0].sum())} of {B} collide")


@pytest.mark.gpu
def test_spec_tiles(tmp_path):
    """2^21 + 2^19 + 37 rows run as tiles of 2^20 on two alternating streams, and, with the queue budget shrunk, with overflowing
    blocks in every tile: the oracle on a strided slice, on 200 rows around each tile boundary and on the last 200 rows."""
    import torch
    from numbotics_amd._lib import debug_option
    from numbotics_amd.parallel import unpack_mask
    arm, chain, obs, sm, dev, orc = _edge_scene("c2", str(tmp_path))
    tile = 1 << 20
    B = 2 * tile + (1 << 19) + 37
    qh = sc.sample(chain, B, 61)
    q = torch.from_numpy(qh).cuda()
    sl = np.unique(np.concatenate([np.arange(0, B, 211), np.arange(tile - 100, tile + 100), np.arange(2 * tile - 100, 2 * tile + 100),
                                   np.arange(B - 200, B)]))
    ref = orc.validity(qh[sl], 0.0, nthreads=16)
    got = _validity(dev, q, 0.0, "tiles").cpu().numpy()
    assert np.array_equal(got[sl], ref), sl[got[sl] != ref][:8]
    words = _validity(dev, q, 0.0, "tiles packed", packed=True).cpu().numpy()
    assert np.array_equal(unpack_mask(words, B), got)
    with debug_option("queue_budget", 1 << 17):
        assert np.array_equal(_validity(dev, q, 0.0, "tiles, small queue").cpu().numpy(), got)
    print(f"tiles: {B} rows served by kernel {sc.used_kernel(dev)}; {int(ref.sum())} of {sl.size} checked rows collide")


@pytest.mark.gpu
def test_spec_two_streams_and_a_small_call_in_between(tmp_path):
    """Two streams share one descriptor without synchronising, both served by the specialised kernel; then a call of 4 096 rows
    between two large ones: the generic kernel serves it, the specialised one the next large call on the same descriptor."""
    import torch
    arm, chain, obs, sm, dev, orc = _edge_scene("c2", str(tmp_path))
    B = sc.SPEC_MIN_BATCH + 37
    qh = sc.sample(chain, 2 * B, 71)
    ref_a, ref_b = orc.validity(qh[:B], 0.0, nthreads=8), orc.validity(qh[B:], 0.0, nthreads=8)
    qa, qb = torch.from_numpy(qh[:B]).cuda(), torch.from_numpy(qh[B:]).cuda()
    _validity(dev, qa, 0.0, "first call")                    # compiles
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for rep in range(4):
        with torch.cuda.stream(s1):
            va = dev.validity(qa, 0.0)
            used_a = sc.used_kernel(dev)
        with torch.cuda.stream(s2):
            vb = dev.validity(qb, 0.0, packed=True)
            used_b = sc.used_kernel(dev)
        outs.append((va, vb, used_a, used_b))
    torch.cuda.synchronize()
    from numbotics_amd.parallel import unpack_mask
    for va, vb, used_a, used_b in outs:
        assert used_a == used_b == sc.SPECIALISED
        assert np.array_equal(va.cpu().numpy(), ref_a) and np.array_equal(unpack_mask(vb.cpu().numpy(), B), ref_b)
    assert np.array_equal(_validity(dev, qh[:B], 0.0, "large call"), ref_a)
    small = dev.validity(qh[B:B + 4096], 0.0)
    assert sc.used_kernel(dev) in (sc.GENERIC, 3)
    assert np.array_equal(small, ref_b[:4096])
    assert np.array_equal(_validity(dev, qh[B:], 0.0, "large call after a small one"), ref_b)
    print(f"streams: large calls served by kernel {sc.used_kernel(dev)}, the small one by the generic kernel")
