"""The held object against point clouds, the part that needs no device: the shares of the GPU tests' fixtures
(tests/held_cloud_cases.py) pinned on the CPU reference alone -- so that no GPU test can pass on a one-sided case --, the argument
rules the six C entry points answer before any device is touched, the two workspace sizes, the header / binding agreement and the
refusals of ``ConnectorParams(attached_sees_cloud=True)``."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from numbotics_amd import _lib
from numbotics_amd.scenes import build_scene, sample_q
import held_cases as hc
import held_cloud_cases as hcc
import held_traj_cases as ht

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nbk_held_cloud_validity_batch", "nbk_held_cloud_clearance_batch", "nbk_edge_held_cloud_workspace_bytes",
           "nbk_edge_held_cloud_validity_batch", "nbk_spline_held_cloud_workspace_bytes", "nbk_spline_held_cloud_validity_batch")
nan, inf = float("nan"), float("inf")


@pytest.fixture()
def c2(fresh_world):
    """Scene c2 with the parity fixtures' box on the gripper -> namespace(arm, chain, keep, sm, att, spec, q, shapes): ``shapes`` the
    robot shapes the connector's arm-versus-scan step checks (the base stands on the scanned table)."""
    arm, chain, obs = build_scene("c2")
    att, b = hc.gripper_box(arm)
    sm = arm.scene_model()
    base = sm.links[sm.rshape_link[0]]._name
    shapes = [k for k in range(sm.n_rshapes) if sm.links[sm.rshape_link[k]]._name != base]
    return types.SimpleNamespace(arm=arm, chain=chain, keep=(obs, b), sm=sm, att=att, spec=att.spec(arm), q=sample_q(chain, 2000, seed=3),
                                shapes=shapes, base=base)


# ---- the fixtures' shares --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("dense", "sparse"))
def test_fixture_rows(c2, name):
    """Reference: dense (1000 points, r = 0.01) 480 of 2000 hit at thr = 0, 243 of the first 1000, 11 of the first 63; sparse (65
    points, r = 0.02) 320 of 2000, 164 of the first 1000."""
    pts, r = hcc.scan(name)
    for thr in hc.THRESHOLDS:
        m = hcc.mask(c2.sm, c2.spec, pts, r, c2.q, thr)
        print(f"{name} thr={thr}: {int(m.sum())} of 2000 hit, {int(m[:1000].sum())} of the first 1000, {int(m[:63].sum())} of the first 63")
        for n in (2000, 1000):
            assert 0.05 <= float(m[:n].mean()) <= 0.95, (name, thr, n, float(m[:n].mean()))
        for B in hcc.BATCHES[1:]:
            assert 0 < m[:B].sum() < B, (name, thr, B)
    if name == "dense":
        m = hcc.mask(c2.sm, c2.spec, pts, r, c2.q, 0.0)
        assert (int(m.sum()), int(m[:1000].sum()), int(m[:63].sum())) == (480, 243, 11)


def test_fixture_clearance(c2):
    """Reference: 131 of the first 200 rows finite at d_max = 0.3 against the dense scan, 43 of them negative."""
    pts, r = hcc.scan("dense")
    d, s, p = hcc.closest(c2.sm, c2.spec, pts, r, c2.q[:200], 0.3)
    fin = np.isfinite(d)
    print(f"clearance: {int(fin.sum())} of 200 finite, {int((d < 0).sum())} negative")
    assert fin.sum() >= 20 and np.isposinf(d).sum() >= 20 and (d < 0).sum() >= 5
    assert (s[fin] == 0).all() and (s[~fin] == -1).all() and (p[fin] >= 0).all() and (p[~fin] == -1).all()


@pytest.mark.parametrize("name", ("dense", "sparse"))
def test_fixture_edges(c2, name):
    """Reference, 200 edges: dense connect 130 valid, 33 that arm-versus-scan alone accepts and the held box rejects; sparse connect
    148 and 26; steer (max_distance 0.4) 147 valid dense, 164 sparse."""
    pts, r = hcc.scan(name)
    s, g = hc.edge_set(c2.q, hcc.N_EDGES)
    e = hcc.edges_ref(c2.sm, c2.spec, pts, r, s, g, hcc.MAXD)
    a = hcc.arm_cloud_edges_ref(c2.sm, pts, r, s, g, hcc.MAXD, shapes=c2.shapes)
    silent = int((a[0] & ~e[0]).sum())
    print(f"{name} connect: {int(e[0].sum())} of 200 valid, {silent} accepted by arm-versus-scan and rejected by the held box")
    assert e[0].sum() >= 10 and (~e[0]).sum() >= 10 and silent >= 3
    st = hcc.edges_ref(c2.sm, c2.spec, pts, r, s, g, hcc.MAXD_STEER, "steer")
    print(f"{name} steer: {int(st[0].sum())} of 200 valid")
    assert 0 < st[0].sum() < hcc.N_EDGES
    for E in hcc.EDGE_COUNTS[1:]:
        assert 0 < e[0][:E].sum() < E and 0 < st[0][:E].sum() < E, (name, E)


def test_fixture_splines(c2):
    """Reference: of the 65 degree-3 splines 52 are valid against the dense scan and 56 against the sparse one."""
    ctrl, knots = ht.splines(c2, 3)
    for name in ("dense", "sparse"):
        pts, r = hcc.scan(name)
        v, t, ns = hcc.splines_ref(c2.sm, c2.spec, pts, r, ctrl, knots, 3)
        print(f"splines, {name}: {int(v.sum())} of 65 valid")
        assert 0 < v.sum() < 65 and 0 < v[:64].sum() < 64
        assert np.isnan(t[v]).all() and np.isfinite(t[~v]).all() and (ns > 0).all()


def test_fixture_grasp_rows(c2):
    """Reference: of 64 rows each with its own grasp (held_cases.rot_pose, rng seed 1) 11 hit the dense scan."""
    pts, r = hcc.scan("dense")
    rng = np.random.default_rng(1)
    G = np.array([hc.rot_pose(rng) for _ in range(64)])
    m = hcc.mask_rows(c2.sm, c2.spec, pts, r, c2.q[:64], 0.0, G)
    print(f"64 grasps: {int(m.sum())} hit")
    assert 0 < m.sum() < 64


# ---- the C boundary ----------------------------------------------------------------------------------------------------------------
def test_symbols_declared_and_bound():
    with open(os.path.join(ROOT, "include", "nbk.h")) as f:
        text = f.read()
    declared = set(re.findall(r"\b(nbk_\w+)\s*\(", text))
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in declared and s in _lib.SYMBOLS and hasattr(lib, s), s
    assert re.search(r"#define\s+NBK_ABI_VERSION\s+2\b", text), "additions only: the ABI version stays 2"


def test_workspace_sizes_are_the_cloud_siblings():
    from numbotics_amd.engine import DeviceModel
    lib = _lib.load()
    assert lib.nbk_edge_held_cloud_workspace_bytes(-1) < 0 and lib.nbk_spline_held_cloud_workspace_bytes(-1) < 0
    for n in (0, 1, 63, 64, 65, 200, 100000):
        assert lib.nbk_edge_held_cloud_workspace_bytes(n) == lib.nbk_edge_cloud_workspace_bytes(n) >= 40 * n
        assert lib.nbk_spline_held_cloud_workspace_bytes(n) == lib.nbk_spline_cloud_workspace_bytes(n) > 0 or n == 0
        assert DeviceModel.held_cloud_edge_workspace_bytes(n) == lib.nbk_edge_cloud_workspace_bytes(n)
        assert DeviceModel.held_cloud_spline_workspace_bytes(n) == lib.nbk_spline_cloud_workspace_bytes(n)
    assert lib.nbk_spline_held_cloud_workspace_bytes(2**26) == lib.nbk_spline_cloud_workspace_bytes(2**26) == -1


def _buffers():
    """Non-null stand-ins: ``fake`` (zeroed, 4096 bytes) for the three handles -- a held object whose descriptor field reads null is
    "made against another descriptor" --, ``base`` a 64-byte aligned address for every array."""
    fake = (C.c_char * 4096)()
    other = (C.c_char * 4096)()
    mem = np.zeros((1 << 16,), dtype=np.uint8)
    base = mem.ctypes.data + (-mem.ctypes.data) % 64
    return C.addressof(fake), C.addressof(other), base, (fake, other, mem)


ROWS = ("m", "held", "c", "q", "B", "grasp", "grasp_rows")


def _rows(lib, which, **kw):
    f, o, base, keep = _buffers()
    a = dict(m=f, held=o, c=f, q=base, B=8, grasp=None, grasp_rows=0, threshold=0.0, accumulate=0, mask_bits=None, mask_bytes=base,
             d_max=0.3, min_dist=base, shape=None, point=None, stream=None)
    a.update(kw)
    if which == "validity":
        order = ROWS + ("threshold", "accumulate", "mask_bits", "mask_bytes", "stream")
        return lib.nbk_held_cloud_validity_batch(*[a[k] for k in order])
    order = ROWS + ("d_max", "min_dist", "shape", "point", "stream")
    return lib.nbk_held_cloud_clearance_batch(*[a[k] for k in order])


def test_row_entries_argument_rules_need_no_device():
    lib = _lib.load()
    f, o, base, keep = _buffers()
    shared = {"null descriptor": dict(m=None), "null held object": dict(held=None), "null cloud": dict(c=None), "negative B": dict(B=-1),
              "null q": dict(q=None), "grasp_rows 7": dict(grasp=base, grasp_rows=7), "grasp_rows -1": dict(grasp=base, grasp_rows=-1),
              "rows without a grasp": dict(grasp_rows=1), "a grasp without rows": dict(grasp=base),
              "rows B without a grasp": dict(grasp_rows=8)}
    bad = {"validity": dict(shared, **{"NaN threshold": dict(threshold=nan), "no mask": dict(mask_bytes=None)}),
           "clearance": dict(shared, **{"NaN d_max": dict(d_max=nan), "+inf d_max": dict(d_max=inf), "-inf d_max": dict(d_max=-inf),
                                        "null min_dist": dict(min_dist=None)})}
    for which, cases in bad.items():
        for what, kw in cases.items():
            assert _rows(lib, which, **kw) == -1, f"{which}: {what}"
        # past its own rules the call asks whose the held object is, before any device: the stand-in belongs to no descriptor
        for kw in (dict(), dict(grasp=base, grasp_rows=1), dict(grasp=base, grasp_rows=8), dict(B=0)):
            assert _rows(lib, which, **kw) == -1, f"{which}: a held object made against another descriptor {kw}"
            assert "another descriptor" in lib.nbk_last_error().decode(), which
    assert _rows(lib, "validity", mask_bits=base, mask_bytes=None) == -1 and "another descriptor" in lib.nbk_last_error().decode()
    del keep, f, o


EDGE_ORDER = ("m", "held", "c", "starts", "goals", "dist", "E", "resolution", "max_distance", "mode", "threshold", "grasp", "accumulate",
              "valid", "end", "n_samples", "workspace", "workspace_bytes", "stream")
SPLINE_ORDER = ("m", "held", "c", "ctrl", "S", "n_ctrl", "degree", "knots", "resolution", "threshold", "grasp", "accumulate", "valid",
                "t_hit", "n_samples", "workspace", "workspace_bytes", "stream")


def _traj(lib, which, n=4, **kw):
    f, o, base, keep = _buffers()
    a = dict(m=f, held=o, c=f, resolution=0.05, threshold=0.0, grasp=None, accumulate=0, valid=base, n_samples=None, workspace=base,
             stream=None)
    if which == "edges":
        a.update(starts=base, goals=base, dist=None, E=n, max_distance=0.25, mode=0, end=None,
                 workspace_bytes=lib.nbk_edge_held_cloud_workspace_bytes(max(n, 0)))
    else:
        a.update(ctrl=base, S=n, n_ctrl=6, degree=3, knots=base, t_hit=None,
                 workspace_bytes=lib.nbk_spline_held_cloud_workspace_bytes(max(n, 0)))
    if "workspace_offset" in kw:
        a["workspace"] = base + kw.pop("workspace_offset")
    a.update(kw)
    fn, order = (lib.nbk_edge_held_cloud_validity_batch, EDGE_ORDER) if which == "edges" else (lib.nbk_spline_held_cloud_validity_batch, SPLINE_ORDER)
    return fn(*[a[k] for k in order])


def test_trajectory_entries_argument_rules_need_no_device():
    lib = _lib.load()
    shared = {"null descriptor": dict(m=None), "null held object": dict(held=None), "null cloud": dict(c=None), "null valid": dict(valid=None),
              "null workspace": dict(workspace=None), "resolution 0": dict(resolution=0.0), "resolution NaN": dict(resolution=nan),
              "resolution inf": dict(resolution=inf), "negative resolution": dict(resolution=-0.05), "NaN threshold": dict(threshold=nan),
              "workspace misaligned": dict(workspace_offset=8), "workspace 32-aligned": dict(workspace_offset=32)}
    edges = dict(shared, **{"negative E": dict(E=-1), "null starts": dict(starts=None), "null goals": dict(goals=None),
                            "max_distance 0": dict(max_distance=0.0), "max_distance NaN": dict(max_distance=nan), "mode 2": dict(mode=2),
                            "workspace one byte short": dict(workspace_bytes=lib.nbk_edge_held_cloud_workspace_bytes(4) - 1),
                            "workspace of no bytes": dict(workspace_bytes=0)})
    splines = dict(shared, **{"negative S": dict(S=-1), "null ctrl": dict(ctrl=None), "null knots": dict(knots=None), "degree 0": dict(degree=0),
                              "degree 6": dict(degree=6, n_ctrl=8), "n_ctrl equal to the degree": dict(n_ctrl=3),
                              "workspace one byte short": dict(workspace_bytes=lib.nbk_spline_held_cloud_workspace_bytes(4) - 1),
                              "workspace of no bytes": dict(workspace_bytes=0)})
    for which, cases in (("edges", edges), ("splines", splines)):
        for what, kw in cases.items():
            assert _traj(lib, which, **kw) == -1, f"{which}: {what}"
        assert _traj(lib, which, n=0) == 0, f"{which}: nothing to do is answered before the handles are looked at"
        assert _traj(lib, which, n=0, workspace=None, valid=None, workspace_bytes=0) == 0
        assert _traj(lib, which) == -1 and "another descriptor" in lib.nbk_last_error().decode(), which
    assert _traj(lib, "splines", n=2**26, workspace_bytes=0) == -4, "too many trajectories: unsupported, without a device"


# ---- the public layer ---------------------------------------------------------------------------------------------------------------
def test_attached_sees_cloud_refusals(c2):
    from numbotics_amd.planning.sampling_based.connectors import ConnectorParams, DiscreteConnector, ContinuousConnector
    cloud = object()                                             # (no rule below looks into it)
    assert ConnectorParams(arm=c2.arm).attached_sees_cloud is False
    assert ConnectorParams(arm=c2.arm, cloud=cloud, attached=c2.att).attached_sees_cloud is False, "the default stays False"
    for kw in (dict(arm=c2.arm), dict(arm=c2.arm, cloud=cloud), dict(arm=c2.arm, attached=c2.att),
               dict(validity_checker=lambda q: True)):
        with pytest.raises(ValueError, match="attached_sees_cloud needs"):
            ConnectorParams(attached_sees_cloud=True, **kw)
    p = ConnectorParams(arm=c2.arm, cloud=cloud, attached=c2.att, attached_sees_cloud=True)
    assert p.attached_sees_cloud is True
    DiscreteConnector(p)
    with pytest.raises(ValueError, match="certified held-object checks do not see point clouds yet"):
        ContinuousConnector(p)
    # a trajectory call must still name the scan and the attachment
    con = DiscreteConnector(p)
    with pytest.raises(ValueError, match="do not see held objects yet"):
        con.validate_trajectories(c2.q[None, :4], degree=1)
    with pytest.raises(ValueError, match="do not see point clouds yet"):
        con.validate_trajectories(c2.q[None, :4], degree=1, attached=c2.att)
