"""The trims of the per-robot broadphase (nbk_bf32_spec.hpp: the axis-aligned box slot, q rows loaded straight into registers): the
specialised kernel's masks against the generic kernel's (NBK_NO_JIT=1 in a child process) on every row and against the float64
oracle on a strided sample.  Thresholds at which c2's first slot group is out of static reach (<= 0.01: its wbx entries hold the
"never" defaults) and at which it is live (>= 0.02), aligned, rotated and mixed boxes, a movable cube that is rotated, sent out of reach
and brought back, batches with and without a tail wave, a q view at an 8-byte-aligned base, rows with NaN, +inf and 1e300."""
import os
import subprocess
import sys

import numpy as np
import pytest

import spec_cases as sc
import trim_cases as tc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
B0 = sc.SPEC_MIN_BATCH
# 0.02 and 0.05: group 0 of c2 is live (the static bound of shape 1 is 0.092 m with and 0.017 m without the 0.08 m of margins) while
# most rows are still free; at 0.3 every row collides
THRESHOLDS = (0.0, 1e-6, 0.01, -0.002, 0.3, 0.02, 0.05)
# 1e300 is finite as a double and infinite as a float: the finiteness test must read the double.  The oracle defines that row
# (sin(1e300) exists) but both device broadphases, the generic one included, cull a row whose float32 sweep is not finite, so the row
# is compared with the generic kernel only; it is no multiple of ORACLE_STRIDE.  NaN and +inf collide by definition.
BAD_ROWS = {1000: np.nan, 20001: np.inf, 40002: 1e300}
NON_FINITE_ROWS = [r for r, v in BAD_ROWS.items() if not np.isfinite(v)]
# (scene, thresholds, forms); forms: "b0" the first 2^16 rows, "tail" the first 2^16 + 37, "view" rows 1 .. 2^16 + 37 of the tensor
CASES = (("c2", THRESHOLDS, ("b0", "tail", "view")), ("c2_sharp", THRESHOLDS, ("b0", "tail", "view")),
         ("c2_rot", (0.0, 0.01, 0.05, 0.3), ("tail",)), ("two_box", (0.0, 0.01, 0.05, 0.3), ("tail",)))
MOVES = ("start", "rotated", "away", "back")
MOVE_THRESHOLDS = (0.0, 0.01)
ORACLE_STRIDE = 4


def _rows(form):
    return {"b0": slice(0, B0), "tail": slice(0, B0 + 37), "view": slice(1, B0 + 38)}[form]


def _q(chain, seed):
    q = sc.sample(chain, B0 + 38, seed)
    for i, (row, v) in enumerate(BAD_ROWS.items()):
        q[row, i % q.shape[1]] = v
    return q


def _moved_scene(sm, move):
    """The c2 scene model with its cube at the pose of ``move``."""
    if move == "rotated":
        return tc.with_pose(sm, 0, R=tc.rot_z(0.3))
    if move == "away":
        return tc.with_pose(sm, 0, t=sm.wshape_pose.reshape(-1, 3, 4)[0, :, 3] + np.array([2.0, 0.0, 0.0]))
    return sm


def _masks():
    """{"<scene>|<thr>|<form>": packed mask, "<scene>|used": kernels} of every case, and the same for the movable c2 per move."""
    import torch
    from numbotics_amd.engine import DeviceModel
    out = {}
    for name, thrs, forms in CASES:
        sm, chain = tc.scene(name)
        dev = DeviceModel(sm)
        qt = torch.from_numpy(_q(chain, 11)).cuda()
        used = set()
        for thr in thrs:
            for form in forms:
                view = qt[_rows(form)]
                assert view.is_contiguous() and (form != "view" or view.data_ptr() % 16 == (8 if sm.kin.n_q % 2 else 0))
                out[f"{name}|{thr}|{form}"] = np.packbits(dev.validity(view, thr).cpu().numpy())
                used.add(sc.used_kernel(dev))
        out[f"{name}|used"] = np.array(sorted(used), dtype=np.int32)
    sm, chain = tc.scene("c2")
    dev = DeviceModel(sm, movable=True, world_radius=tc.WORLD_RADIUS)
    qt = torch.from_numpy(_q(chain, 12)).cuda()[:B0 + 37]
    used = set()
    for move in MOVES:
        if move != "start":
            dev.set_world_poses(_moved_scene(sm, move).wshape_pose)
        for thr in MOVE_THRESHOLDS:
            out[f"movable|{move}|{thr}"] = np.packbits(dev.validity(qt, thr).cpu().numpy())
            used.add(sc.used_kernel(dev))
    out["movable|used"] = np.array(sorted(used), dtype=np.int32)
    return out


@pytest.fixture(scope="module")
def generic(tmp_path_factory):
    """The masks of every case from the generic kernel: ONE fresh process with NBK_NO_JIT=1."""
    out = os.path.join(str(tmp_path_factory.mktemp("trim")), "generic.npz")
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {HERE!r}); import numpy as np; import test_gpu_broad_trim as t; "
            f"np.savez({out!r}, **{{k.replace('|', '@'): v for k, v in t._masks().items()}})")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, NBK_NO_JIT="1"), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(out) as z:
        return {k.replace("@", "|"): z[k] for k in z.files}


@pytest.fixture(scope="module")
def mine():
    return _masks()


def _bits(m, n):
    return np.unpackbits(m)[:n].astype(bool)


@pytest.mark.gpu
def test_specialised_kernel_served_every_case(mine, generic):
    for name in [c[0] for c in CASES] + ["movable"]:
        assert mine[f"{name}|used"].tolist() == [sc.SPECIALISED], (name, mine[f"{name}|used"])
        assert generic[f"{name}|used"].tolist() == [sc.GENERIC], (name, generic[f"{name}|used"])


@pytest.mark.gpu
@pytest.mark.parametrize("name,thrs,forms", CASES, ids=[c[0] for c in CASES])
def test_masks_equal_generic_and_oracle(name, thrs, forms, mine, generic):
    from oracle.cpu_oracle import Oracle
    sm, chain = tc.scene(name)
    q = _q(chain, 11)
    orc = Oracle(sm)
    sample = np.unique(np.concatenate([np.arange(0, B0 + 38, ORACLE_STRIDE), np.array(NON_FINITE_ROWS), np.arange(B0 - 2, B0 + 38)]))
    for thr in thrs:
        ref = orc.validity(q[sample], thr, nthreads=8)
        for form in forms:
            rows = _rows(form)
            n = rows.stop - rows.start
            got, gen = _bits(mine[f"{name}|{thr}|{form}"], n), _bits(generic[f"{name}|{thr}|{form}"], n)
            assert np.array_equal(got, gen), f"{name} at {thr}, {form}: specialised != generic in rows {np.flatnonzero(got != gen)[:8].tolist()}"
            inside = (sample >= rows.start) & (sample < rows.stop)
            bad = sample[inside][got[sample[inside] - rows.start] != ref[inside]]
            assert bad.size == 0, f"{name} at {thr}, {form}: != oracle in rows {bad[:8].tolist()}"
            for row in NON_FINITE_ROWS:
                assert got[row - rows.start], (name, thr, form, row)
        print(f"{name} at {thr}: {int(ref.sum())} of {sample.size} sampled rows collide")
    # the dead and the live slot group ran on masks that are not trivial: more rows collide at 0.05 than at 0.01, not all; at 0.3 all do
    n = B0 + 37
    lo, hi = _bits(mine[f"{name}|0.01|tail"], n), _bits(mine[f"{name}|0.05|tail"], n)
    assert 0 < lo.sum() < hi.sum() and not hi.all(), (name, int(lo.sum()), int(hi.sum()))
    assert np.delete(_bits(mine[f"{name}|0.3|tail"], n), 40002).all(), name          # (the 1e300 row: see BAD_ROWS)


@pytest.mark.gpu
def test_movable_cube_rotated_sent_away_and_back(mine, generic):
    from oracle.cpu_oracle import Oracle
    sm, chain = tc.scene("c2")
    q = _q(chain, 12)[:B0 + 37]
    sample = np.unique(np.concatenate([np.arange(0, B0 + 37, ORACLE_STRIDE), np.array(NON_FINITE_ROWS)]))
    count = {}
    for move in MOVES:
        orc = Oracle(_moved_scene(sm, move))
        for thr in MOVE_THRESHOLDS:
            got, gen = _bits(mine[f"movable|{move}|{thr}"], B0 + 37), _bits(generic[f"movable|{move}|{thr}"], B0 + 37)
            assert np.array_equal(got, gen), f"{move} at {thr}: specialised != generic in rows {np.flatnonzero(got != gen)[:8].tolist()}"
            ref = orc.validity(q[sample], thr, nthreads=8)
            assert np.array_equal(got[sample], ref), f"{move} at {thr}: != oracle in rows {sample[got[sample] != ref][:8].tolist()}"
            count[move, thr] = int(got.sum())
    for thr in MOVE_THRESHOLDS:
        assert np.array_equal(mine[f"movable|back|{thr}"], mine[f"movable|start|{thr}"])
        # out of reach, only self collisions are left; the rotated cube gives another mask than the aligned one
        assert count["away", thr] < count["start", thr] and not np.array_equal(mine[f"movable|rotated|{thr}"], mine[f"movable|start|{thr}"])
    print("colliding rows per move and threshold:", count)
