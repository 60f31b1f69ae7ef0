"""Witness points and gradient rows of held items, the part that needs no GPU: the oracle side of the bar the GPU tests
(tests/test_gpu_held_records.py) compare against -- its rows on ``held_model`` are the gradient of its distances --, the new symbols
and their argument rules at the C boundary, the argument rules of the Python front-ends, and, by the reference alone, the conditions
the GPU cases rely on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from numbotics_amd import _lib
import held_cases as hc
import held_cloud_cases as hcc
import held_records_cases as rc
import held_traj_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nbk_held_records_batch", "nbk_held_records_items", "nbk_held_cloud_records_batch")
nan, inf = float("nan"), float("inf")


# ---- 6. the oracle side of the bar -------------------------------------------------------------------------------------------------
def test_oracle_rows_are_the_gradient_on_held_model(fresh_world):
    """On ``held_model`` of c3 the oracle's rows equal central differences of its ``pair_distances`` (h, the separation and the bound
    of tests/test_oracle_proximity.py), for robot items -- subject the link shape, target the held shape -- and world items alike."""
    from oracle.cpu_oracle import Oracle
    x = tc.scene("c3")
    hm = hc.held_model(x.sm, x.spec)
    orc = Oracle(hm)
    q = x.q[:40]
    d, w, rows = orc.proximity_jacobian(q)
    cols = tc.item_columns(x.sm, x.spec)
    assert d.shape == (40, len(cols)) and (cols[:, 1] == 0).any() and (cols[:, 1] == 1).any()
    h = 1e-4
    num = np.zeros_like(rows)
    for j in range(hm.kin.n_q):
        qp, qm = q.copy(), q.copy()
        qp[:, j] += h
        qm[:, j] -= h
        num[:, :, j] = (orc.pair_distances(qp) - orc.pair_distances(qm)) / (2 * h)
    sep = d > 5e-3
    assert sep.mean() > 0.5
    for kind in (0, 1):
        assert sep[:, cols[:, 1] == kind].any(), f"no separated item of kind {kind}"
    err = np.abs(num - rows)[sep]
    print(f"largest difference between the rows and central differences over {int(sep.sum())} separated items: {err.max():.3e}")
    assert err.max() < 2e-5, err.max()
    assert np.abs(rows).max() > 0.1
    # a robot item whose link mask and held mask share joints: a shared joint moves both witness points alike, so its column is
    # n . (w x (p_s - p_t)) = 0 -- p_s - p_t is along n.  In floating point: zero to rounding (the two terms are O(1))
    kin = hm.kin
    def path(f):
        out = set()
        while f >= 0:
            out.add(int(f))
            f = int(kin.joint_parent[f])
        return out
    held_path = path(x.spec.frame)
    seen, moved = 0, 0.0
    for k, (hh, kind, s) in enumerate(cols):
        if kind != 0:
            continue
        shared = sorted(path(int(x.sm.rshape_frame[s])) & held_path)
        if not shared:
            continue
        seen += 1
        c = [int(kin.joint_qidx[j]) for j in shared]
        assert np.abs(rows[:, k][:, c]).max() < 1e-12, (k, np.abs(rows[:, k][:, c]).max())
        rest = [int(kin.joint_qidx[j]) for j in sorted(held_path - set(shared))]
        moved = max(moved, np.abs(rows[:, k][:, rest]).max())
    assert seen >= 3, "robot items that share joints with the holding path"
    assert moved > 0.1, "the joints between a link and the hand do move their distance"


# ---- 7. the C boundary -------------------------------------------------------------------------------------------------------------
def test_symbols_declared_and_bound():
    with open(os.path.join(ROOT, "include", "nbk.h")) as f:
        text = f.read()
    declared = set(re.findall(r"\b(nbk_\w+)\s*\(", text))
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/nbk.h"
        assert s in _lib.SYMBOLS, f"{s} is not listed in _lib.SYMBOLS"
        assert hasattr(lib, s), f"libnbk.so lacks {s}"
        assert getattr(lib, s).argtypes is not None, f"{s} has no argtypes"
    assert re.search(r"#define\s+NBK_ABI_VERSION\s+2\b", text), "additions only: the ABI version stays 2"


def _buffers():
    """Non-null stand-ins, as tests/test_held_cloud_host.py has them: zeroed blocks for the handles -- a held object whose descriptor
    field reads null is "made against another descriptor" --, ``base`` a 64-byte aligned address for every array."""
    fake = (C.c_char * 4096)()
    other = (C.c_char * 4096)()
    mem = np.zeros((1 << 16,), dtype=np.uint8)
    base = mem.ctypes.data + (-mem.ctypes.data) % 64
    return C.addressof(fake), C.addressof(other), base, (fake, other, mem)


ORDER = {"batch": ("m", "held", "q", "B", "grasp", "grasp_rows", "dist", "witness", "jrows", "stream"),
         "items": ("m", "held", "q", "B", "items", "N", "grasp", "grasp_rows", "dist", "witness", "jrows", "stream"),
         "cloud": ("m", "held", "c", "q", "B", "grasp", "grasp_rows", "d_max", "per_shape", "dist", "shape", "point", "witness", "jrows",
                   "stream")}


def _call(lib, which, **kw):
    f, o, base, keep = _buffers()
    a = dict(m=f, held=o, c=f, q=base, B=8, items=base, N=5, grasp=None, grasp_rows=0, d_max=0.3, per_shape=0, dist=base, shape=None,
             point=None, witness=None, jrows=None, stream=None)
    a.update(kw)
    fn = {"batch": lib.nbk_held_records_batch, "items": lib.nbk_held_records_items, "cloud": lib.nbk_held_cloud_records_batch}[which]
    return fn(*[a[k] for k in ORDER[which]])


def test_argument_rules_need_no_device():
    lib = _lib.load()
    f, o, base, keep = _buffers()
    shared = {"null descriptor": dict(m=None), "null held object": dict(held=None), "negative B": dict(B=-1), "null q": dict(q=None),
              "null dist": dict(dist=None), "grasp_rows 7": dict(grasp=base, grasp_rows=7), "grasp_rows -1": dict(grasp=base, grasp_rows=-1),
              "rows without a grasp": dict(grasp_rows=1), "a grasp without rows": dict(grasp=base),
              "rows B without a grasp": dict(grasp_rows=8)}
    bad = {"batch": shared,
           "items": dict(shared, **{"negative N": dict(N=-1), "null items": dict(items=None)}),
           "cloud": dict(shared, **{"null cloud": dict(c=None), "NaN d_max": dict(d_max=nan), "+inf d_max": dict(d_max=inf),
                                    "-inf d_max": dict(d_max=-inf)})}
    for which, cases in bad.items():
        for what, kw in cases.items():
            assert _call(lib, which, **kw) == -1, f"{which}: {what}"
        # past its own rules the call asks whose the held object is, before any device: the stand-in belongs to no descriptor
        for kw in (dict(), dict(grasp=base, grasp_rows=1), dict(grasp=base, grasp_rows=8), dict(witness=base, jrows=base), dict(B=0)):
            assert _call(lib, which, **kw) == -1, f"{which}: a held object made against another descriptor {kw}"
            assert "another descriptor" in lib.nbk_last_error().decode(), which
    assert _call(lib, "items", N=0, items=None, dist=None) == -1 and "another descriptor" in lib.nbk_last_error().decode(), \
        "N = 0 needs neither items nor dist"
    assert _call(lib, "cloud", per_shape=1) == -1 and "another descriptor" in lib.nbk_last_error().decode()
    del keep, f, o


# ---- the Python front-ends: errors raised before any device call ----------------------------------------------------------------------
def test_front_end_errors_come_before_the_device(fresh_world):
    from numbotics_amd.engine import DeviceModel
    from numbotics_amd.physics import Cuboid
    from numbotics_amd.planning import safe_sets
    from numbotics_amd.scenes import build_scene
    x = tc.scene("c3")
    q = x.q[:4]
    calls = (lambda q_, att: x.arm.attached_proximity_jacobians(q_, att),
             lambda q_, att: x.arm.attached_proximity_jacobians(q_, att, per_item=True),
             lambda q_, att: x.arm.attached_cloud_proximity_jacobians(q_, att, object(), 0.1))
    for f in calls:
        with pytest.raises(ValueError, match="elements"):
            f(q[:, :5], x.att)
        with pytest.raises(ValueError, match="must be an Attachment"):
            f(q, x.keep[1])
    for f in (lambda q_, att: x.arm.attached_closest_to(q_, att), lambda q_, att: x.arm.attached_cloud_closest_to(q_, att, object(), 0.1)):
        with pytest.raises(ValueError, match="1D array"):
            f(q, x.att)
        with pytest.raises(ValueError, match="must be an Attachment"):
            f(q[0], "box")
    with pytest.raises(ValueError, match="must be an Attachment"):
        safe_sets.attached_distance_and_gradient(x.arm, q, None)
    # an attachment that does not resolve against this arm: its link belongs to another chain; a touch link nobody knows
    other, chain2, obs2 = build_scene("c1")
    foreign = other.attach(Cuboid(0.0, np.array([0.02, 0.02, 0.02]), position=hc.PARK.copy()), "gripper", pose=hc.trans(0, 0, 0.1))
    from numbotics_amd.physics import Attachment
    unknown = Attachment(x.att.link, x.att.objects, x.att.pose, touch_links=("no_such_link",))
    for f in calls:
        with pytest.raises(ValueError, match="not found in chain"):
            f(q, foreign)
        with pytest.raises(ValueError, match="not found in chain"):
            f(q, unknown)
    # the engine's own rules: whose the held object is, and the form of ``items``, before the device is asked for
    dev = DeviceModel.__new__(DeviceModel)
    for f in (lambda: DeviceModel.held_records(dev, "held", q), lambda: DeviceModel.held_closest_records(dev, None, q),
              lambda: DeviceModel.held_cloud_records(dev, object(), object(), q, 0.1)):
        with pytest.raises(ValueError, match="must be a DeviceHeld"):
            f()
    for items in (np.zeros((3, 3), dtype=np.int32), np.zeros((4,), dtype=np.int32), np.zeros((3, 2)), np.zeros((3, 2), dtype=bool)):
        with pytest.raises(ValueError, match=r"\(N, 2\) integer"):
            DeviceModel._check_items(items)
    DeviceModel._check_items(np.zeros((0, 2), dtype=np.int64))
    DeviceModel._check_items([[0, 1], [2, 3]])
    del obs2, dev


# ---- the conditions the GPU cases rely on, by the reference alone ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("c3", "c2", "c1"))
def test_fixture_conditions_items(fresh_world, name):
    x = tc.scene(name)
    x.q = x.q[:rc.N_ROWS]
    d, w, rows = rc.item_ref(x, name, None)
    cols = tc.item_columns(x.sm, x.spec)
    closest = cols[d.argmin(axis=1), 1]
    print(f"{name}: K = {len(cols)}, {int((d < 0).sum())} penetrating of {d.size}, largest |row| {np.abs(rows).max():.3f}, "
          f"closest item a robot item in {int((closest == 0).sum())} of {len(closest)} rows")
    assert (d < 0.0).any() and (d > 0.0).any() and np.abs(rows).max() > 0.1
    assert len(set(d.argmin(axis=1).tolist())) >= 3
    if name == "c3":
        assert (closest == 0).any() and (closest == 1).any(), "a robot item and a world item are the closest somewhere"
    if name == "c1":
        assert (cols[:, 1] == 0).all()
    for k in range(4):
        assert rc.item_ref(x, name, k)[0].tobytes() != d.tobytes(), "the grasps change the records"


@pytest.mark.parametrize("scan", ("dense", "sparse"))
def test_fixture_conditions_cloud(fresh_world, scan):
    x = rc.eight_scene()
    raw = rc.cloud_raw(x, scan)
    d, s, p, w, j = rc.cloud_ref(x, raw, rc.D_MAX[scan], False)
    near = np.isfinite(d)
    print(f"{scan}: {int(near.sum())} of {len(d)} rows within d_max = {rc.D_MAX[scan]}, {int((d[near] < 0).sum())} penetrating, winning "
          f"held shapes {sorted(set(s[near].tolist()))}")
    assert near.sum() >= 10 and (~near).sum() >= 10 and len(set(s[near].tolist())) >= 3 and (d[near] < 0).any()
    assert not j[~near].view(np.int64).any() and np.isnan(w[~near]).all()
    ds, ss, ps, ws, js = rc.cloud_ref(x, raw, rc.D_MAX[scan], True)
    assert ds.shape == (rc.N_ROWS, 8) and set(ss[np.isfinite(ds)].tolist()) <= set(range(8))
    assert (np.isfinite(ds).sum(axis=0) > 0).sum() >= 3, "at least three columns have winners"


def test_fixture_conditions_graph(fresh_world):
    """The clouds and grasps of the captured graph of tests/test_gpu_held_records.py: each replay is a mixed case, and they differ."""
    import cloud_cases as cc
    x = rc.eight_scene()
    rng = np.random.default_rng(3)
    Gs = [x.spec.G @ hc.rot_pose(rng, 0.3, 0.02) @ hc.trans(0, 0, -hc.BOX_Z) for _ in range(3)]
    seen = set()
    for k, seed in ((1, 41), (2, 42)):
        pts = np.ascontiguousarray(cc.scan(1000, seed=seed))
        d = rc.cloud_ref(x, rc.cloud_raw_of(x, pts, 0.01, x.q, Gs[k]), 0.1, False)[0]
        near = np.isfinite(d)
        print(f"replay {k}: {int(near.sum())} of {len(d)} rows near")
        assert near.sum() >= 5 and (~near).sum() >= 5
        seen.add(d.tobytes())
    assert len(seen) == 2
