"""CPU tier of the broadphase-trim tests: the ``wbox_aligned`` member of the generated ``struct Spec`` (csrc/nbk_tables.hpp) -- 1 only
for a box of an immovable descriptor whose rotation is exactly the identity -- and hipRTC compiling every such source for gfx950,
also with each of the kernel's compile-time switches.  No device is needed; the masks are tests/test_gpu_broad_trim.py."""
import numpy as np
import pytest

import spec_cases as sc
import trim_cases as tc
from numbotics_amd.engine import broad_spec_source


@pytest.fixture(scope="module")
def sources():
    out = {}
    for name in tc.SCENES:
        sm, chain = tc.scene(name)
        out[name] = (sm, broad_spec_source(sm))
    sm = out["c2"][0]
    out["c2_movable"] = (sm, broad_spec_source(sm, movable=True, world_radius=tc.WORLD_RADIUS))
    return out


def test_aligned_flag(sources):
    for name, (sm, src) in sources.items():
        assert src is not None, name
        spec = sc.parse_spec(src)
        sc.check_spec(spec, sc.expected_spec(sm), name)
        want = [0] if name == "c2_movable" else tc.ALIGNED[name]
        assert spec["wbox_aligned"] == want, (name, spec["wbox_aligned"], want)
        assert len(spec["wbox_aligned"]) == spec["NW"]
    # what the flag stands on: the rotation of c2's cube is the identity to the last bit, and the movable source differs in it alone
    sm = sources["c2"][0]
    assert np.array_equal(sm.wshape_pose.reshape(-1, 3, 4)[0, :, :3], np.eye(3))
    a, b = sources["c2"][1].decode().splitlines(), sources["c2_movable"][1].decode().splitlines()
    diff = [(x, y) for x, y in zip(a, b) if x != y]
    # (a movable descriptor's reach covers world_radius, so its slack constants differ as well)
    assert len(a) == len(b) and all("wbox_aligned" in x or "f_reach" in x for x, y in diff) and any("wbox_aligned" in x for x, y in diff), diff


def test_a_rotation_off_by_one_ulp_is_not_aligned(sources):
    sm = sources["c2"][0]
    R = np.eye(3)
    R[0, 0] = np.float32(1.0) - np.float32(2.0 ** -24)          # the largest float32 below 1: the float table is what the kernel reads
    spec = sc.parse_spec(broad_spec_source(tc.with_pose(sm, 0, R=R)))
    assert spec["wbox_aligned"] == [0]
    R = np.eye(3)
    R[0, 1] = 1e-30
    assert sc.parse_spec(broad_spec_source(tc.with_pose(sm, 0, R=R)))["wbox_aligned"] == [0]
    # a half turn about z is axis-aligned too, but not the identity: it keeps the general form
    assert sc.parse_spec(broad_spec_source(tc.with_pose(sm, 0, R=np.diag([-1.0, -1.0, 1.0]))))["wbox_aligned"] == [0]


def test_every_source_compiles_for_gfx950(sources):
    L = sc.lib()
    for name, (sm, src) in sources.items():
        assert L.nbk_jit_compile(src, b"gfx950") > 0, (name, L.nbk_last_error())


SWITCHES = ("NBK_SPEC_NO_ALIGNED", "NBK_SPEC_NO_QREG", "NBK_SPEC_DIAG_NO_WORLD", "NBK_SPEC_DIAG_NO_RR", "NBK_SPEC_DIAG_NO_ENQUEUE")


def test_every_switch_compiles(sources, monkeypatch):
    """Each compile-time switch of nbk_bf32_spec.hpp alone, and the two trims off together (several options in one NBK_JIT_OPTIONS,
    separated by blanks), on c2."""
    L = sc.lib()
    src = sources["c2"][1]
    for opt in [f"-D{s}" for s in SWITCHES] + [" ".join(f"-D{s}" for s in SWITCHES[:2])]:
        monkeypatch.setenv("NBK_JIT_OPTIONS", opt)
        assert L.nbk_jit_compile(src, b"gfx950") > 0, (opt, L.nbk_last_error())
    monkeypatch.setenv("NBK_JIT_OPTIONS", "-DNBK_SPEC_NO_QREG  -DNBK_SPEC_WAVES=no_such_name")
    assert L.nbk_jit_compile(src, b"gfx950") < 0
