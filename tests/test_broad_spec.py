"""The float32 broadphase compiled per robot (numbotics_amd/csrc/nbk_bf32_spec.hpp): its masks against the generic kernel's
(NBK_NO_JIT=1 in a child process) and the oracle, rebuilds after pair / world changes, the fall-back when hipRTC fails, graph
replay.  The first test needs no GPU: it compiles the generated source for gfx950 with hipRTC."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from numbotics_amd.scenes import build_scene, sample_q

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
THRESHOLDS = (0.0, 1e-6, 0.01, -0.002)
B = 1 << 16
GENERIC, SPECIALISED = 1, 2


def _lib():
    from numbotics_amd import _lib as L
    lib = L.load()
    lib.nbk_broad_spec_source.restype = C.c_int64
    lib.nbk_broad_spec_source.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    lib.nbk_jit_compile.restype = C.c_int64
    lib.nbk_jit_compile.argtypes = [C.c_char_p, C.c_char_p]
    lib.nbk_broad_kernel_used.restype = C.c_int32
    lib.nbk_broad_kernel_used.argtypes = [C.c_void_p]
    return lib


def _fresh():
    from numbotics_amd.physics import World
    from numbotics_amd.physics.world import _reset_worlds
    _reset_worlds()
    World()


def _spec_source(sm):
    from numbotics_amd.engine import model_desc
    lib = _lib()
    d, keep = model_desc(sm)
    n = lib.nbk_broad_spec_source(C.byref(d), None, 0)
    if n <= 0:
        return n, None
    buf = C.create_string_buffer(int(n))
    assert lib.nbk_broad_spec_source(C.byref(d), buf, n) == n
    del keep
    return n, buf.value


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
