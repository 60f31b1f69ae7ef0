"""CPU tier of the folded-table tests of the per-robot broadphase: the class arrays ``fc_pk`` / ``fc_tl`` / ``fc_any`` of
the generated ``struct Spec`` (csrc/nbk_tables.hpp) against an independent restatement from the scene model, the thresholds of the
classes, hipRTC compiling every source for gfx950 with and without ``NBK_SPEC_NO_FOLD``, and the static ISA of the c2 kernel.  No
device is needed; the masks are tests/test_gpu_broad_fold.py."""
import os
import re
import subprocess

import pytest

import fold_cases as fc
import spec_cases as sc
from numbotics_amd.engine import broad_spec_source

KEYS = ("c2", "c2_sharp", "c2m", "c2_base") + tuple(fc.FOLD_ROBOTS) + tuple(range(len(sc.SPEC_CASES)))


@pytest.fixture(scope="module")
def sources(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("fold_src"))
    out = {}
    for key in KEYS:
        sm, chain = fc.case_model(key, tmp)
        out[key] = (sm, broad_spec_source(sm))
    return out


def _rot(spec, k):
    return spec["fc_pk"][18 * k:18 * k + 15]


def test_class_arrays_follow_the_model(sources):
    folded = 0
    for key, (sm, src) in sources.items():
        assert src is not None, key
        spec = sc.parse_spec(src)
        sc.check_spec(spec, sc.expected_spec(sm), str(key))
        exp = fc.expected_classes(sm, src)
        for name in ("fc_pk", "fc_tl", "fc_any"):
            assert spec[name] == exp[name], (key, name, spec[name], exp[name])
        assert len(spec["fc_pk"]) == 18 * spec["J"] and len(spec["fc_tl"]) == 3 * spec["S"]
        folded += spec["fc_any"]
    assert folded >= 10, folded
    # c2: every joint turns about z and no rotation entry of any joint is a general number; every translation and every shape
    # offset has x = 0.  A movable descriptor keeps the classes: the robot's tables are never rewritten.
    c2 = sc.parse_spec(sources["c2"][1])
    for k in range(c2["J"]):
        assert fc.GEN not in _rot(c2, k), (k, _rot(c2, k))
        assert c2["fc_pk"][18 * k + 15] == fc.ZERO
    assert all(c == fc.ZERO for c in c2["fc_tl"][0::3])
    assert c2["fc_any"] == 1
    mov = sc.parse_spec(broad_spec_source(sources["c2"][0], movable=True, world_radius=4.0))
    assert [mov[n] for n in ("fc_pk", "fc_any")] == [c2[n] for n in ("fc_pk", "fc_any")]
    # random rpy: joints about coordinate axes (kinds 0-2) none of whose entries is folded, and nothing else either
    rnd = sc.parse_spec(sources["rpy_random"][1])
    assert all(kd <= 2 for kd in rnd["jkind"]) and rnd["fc_any"] == 0 and not any(rnd["fc_pk"]) and not any(rnd["fc_tl"])
    # origins at multiples of pi / 2: kinds 0 and 1 without a general rotation entry; a moved base changes no class
    xy = sc.parse_spec(sources["xy_half_pi"][1])
    assert sorted(set(xy["jkind"])) == [0, 1] and all(fc.GEN not in _rot(xy, k) for k in range(xy["J"]))
    mixed = sc.parse_spec(sources["mixed"][1])
    assert mixed["jkind"] == [2, sc.JK_PRISMATIC, 1, sc.JK_GENERIC, 0, 2] and mixed["fc_any"] == 1
    assert sc.parse_spec(sources["c2_base"][1])["fc_pk"] == c2["fc_pk"]
    assert sc.parse_spec(sources["base_shapes"][1])["sh_begin"][1] == 2


def test_class_thresholds(sources):
    """2^-41 is a zero, 2^-39 and -1 + 2^-24 are general numbers (entries of M2 of joint 1 of c2: the float table is what the kernel
    reads); a table value out of the range the folded sweep's overflow argument assumes turns every class off."""
    sm = sources["c2"][0]
    base = sc.parse_spec(sources["c2"][1])["fc_pk"]
    # joint_rot entry 18 + 3 r + col is M2[r][col]; joint 1 turns about z (U = 0, V = 1): m2p[2 r + col] = M2[r][col]
    for value, want in ((2.0 ** -41, fc.ZERO), (-2.0 ** -41, fc.ZERO), (2.0 ** -40, fc.ZERO), (2.0 ** -39, fc.GEN), (-1.0 + 2.0 ** -24, fc.GEN),
                        (1.0, fc.ONE), (-1.0, fc.NEG)):
        got = sc.parse_spec(broad_spec_source(fc.with_joint_rot(sm, 1, 18 + 3 * 1 + 0, value)))["fc_pk"]
        assert got[18 + 2] == want, (value, got[18 + 2], want)
        assert got[:18 + 2] == base[:18 + 2] and got[18 + 3:] == base[18 + 3:], value
    off = sc.parse_spec(broad_spec_source(fc.with_joint_rot(sm, 1, 18 + 3 * 1 + 0, 2.5)))
    assert off["fc_any"] == 0 and not any(off["fc_pk"]) and not any(off["fc_tl"])


def test_every_source_compiles_with_and_without_folding(sources, monkeypatch):
    L = sc.lib()
    for opt in ("", "-DNBK_SPEC_NO_FOLD"):
        monkeypatch.setenv("NBK_JIT_OPTIONS", opt)
        for key, (sm, src) in sources.items():
            assert L.nbk_jit_compile(src, b"gfx950") > 0, (key, opt, L.nbk_last_error())
    # the parts of the folded sweep alone (measurement switches)
    for bits in (1, 2):
        monkeypatch.setenv("NBK_JIT_OPTIONS", f"-DNBK_SPEC_FOLD_PARTS={bits}")
        for key in ("c2", "c2_base", "mixed", "base_shapes"):
            assert L.nbk_jit_compile(sources[key][1], b"gfx950") > 0, (key, bits, L.nbk_last_error())


def _isa(src, tmp, *defines):
    """The gfx950 assembly of a generated source, compiled as build.py compiles the library."""
    from numbotics_amd.csrc import build as hip_build
    path = os.path.join(tmp, "k.hip")
    with open(path, "wb") as f:
        f.write(src)
    flags = [x for x in hip_build.FLAGS if x not in ("-shared", "-fPIC")]
    out = os.path.join(tmp, "k" + "".join(defines) + ".s")
    r = subprocess.run([hip_build.hipcc(), *flags, "--cuda-device-only", "-include", "hip/hip_runtime.h", "-S", *defines, path, "-o", out],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out) as f:
        return f.read()


def _count(text, pattern):
    return len(re.findall(pattern, text, flags=re.M))


def test_static_isa_of_c2(sources, tmp_path):
    """The folded build of c2 keeps 5 waves per SIMD and no scratch, and its folded sweep is the shorter arm: the build holds both
    sweeps, so it is longer than the unfolded build by less than the unfolded sweep it would otherwise repeat."""
    src = sources["c2"][1]
    new, old = _isa(src, str(tmp_path)), _isa(src, str(tmp_path), "-DNBK_SPEC_NO_FOLD")
    for text in (new, old):
        assert re.search(r"; Occupancy: 5\b", text) and re.search(r"; ScratchSize: 0\b", text)
    valu_new, valu_old = _count(new, r"^\s+v_"), _count(old, r"^\s+v_")
    sins_new, sins_old = _count(new, r"^\s+v_sin_f32"), _count(old, r"^\s+v_sin_f32")
    print(f"static VALU: folded build {valu_new} (both sweeps), unfolded build {valu_old}; v_sin_f32 {sins_new} / {sins_old}")
    assert sins_old == 7 and sins_new == 14
    # the unfolded sweep is 338 static VALU; the folded one adds 184 to the build
    assert 0 < valu_new - valu_old < 250, (valu_new, valu_old)
