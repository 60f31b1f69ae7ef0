"""The folded tables of the per-robot broadphase (nbk_bf32_spec.hpp: zeros and +-1 of the robot's tables folded into the chain
sweep): the masks of the folded build against the same kernel compiled with NBK_SPEC_NO_FOLD and against the generic kernel
(NBK_NO_JIT=1), each in ONE child process, on every row, and against the float64 oracle on a strided sample.  c2 in both shape
modes, robots with nothing to fold, with joints about x and y at multiples of pi / 2, with a prismatic and a general-axis joint
between folded ones, on a moved base and with shapes on the base; B = 2^16 + 37 (the specialised kernel and a tail wave).  Rows
whose float32 sweep is not finite (NaN, +inf, 1e300) or leaves the folded sweep's range (1e30), in every joint column, each in a
wave of ordinary rows: such a wave runs the unfolded sweep, whose NaN the generic kernel has too."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fold_cases as fc
import spec_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
B = sc.FUZZ_B
CASES = ("c2", "c2_sharp", "rpy_random", "xy_half_pi", "mixed", "c2_base", "base_shapes")
FOLDED = {"c2": 1, "c2_sharp": 1, "rpy_random": 0, "xy_half_pi": 1, "mixed": 1, "c2_base": 1, "base_shapes": 1}
BAD_VALUES = (np.nan, np.inf, 1e300, 1e30)
ORACLE_STRIDE = 8


def _bad_rows(nq):
    """{row: (column, value)}: every bad value in every joint column, each row in a wave of its own among ordinary rows."""
    rows = {}
    for i, v in enumerate(BAD_VALUES):
        for j in range(nq):
            rows[64 * (3 + 31 * (i * nq + j)) + (7 * i + 11 * j) % 64] = (j, v)
    assert max(rows) < B - 37 and len({r // 64 for r in rows}) == len(rows)
    return rows


def _q(key, chain):
    q = sc.sample(chain, B, 21)
    if key == "c2_bad":
        for row, (j, v) in _bad_rows(q.shape[1]).items():
            q[row, j] = v
    return q


def _masks(tmp):
    """{"<case>|<thr>": packed mask, "<case>|used": kernels}; "c2_bad" is c2 with the bad rows."""
    import torch
    from numbotics_amd.engine import DeviceModel
    out = {}
    for key in CASES + ("c2_bad",):
        sm, chain = fc.case_model("c2" if key == "c2_bad" else key, tmp)
        dev = DeviceModel(sm)
        qt = torch.from_numpy(_q(key, chain)).cuda()
        used = set()
        for thr in sc.THRESHOLDS:
            out[f"{key}|{thr}"] = np.packbits(dev.validity(qt, thr).cpu().numpy())
            used.add(sc.used_kernel(dev))
        out[f"{key}|used"] = np.array(sorted(used), dtype=np.int32)
    return out


def _child(tmp_path_factory, name, env):
    tmp = str(tmp_path_factory.mktemp("fold_" + name))
    out = os.path.join(tmp, name + ".npz")
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {HERE!r}); import numpy as np; import test_gpu_broad_fold as t; "
            f"np.savez({out!r}, **{{k.replace('|', '@'): v for k, v in t._masks({tmp!r}).items()}})")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(out) as z:
        return {k.replace("@", "|"): z[k] for k in z.files}


@pytest.fixture(scope="module")
def unfolded(tmp_path_factory):
    return _child(tmp_path_factory, "unfolded", {"NBK_JIT_OPTIONS": "-DNBK_SPEC_NO_FOLD"})


@pytest.fixture(scope="module")
def generic(tmp_path_factory):
    return _child(tmp_path_factory, "generic", {"NBK_NO_JIT": "1"})


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("fold_mine"))


@pytest.fixture(scope="module")
def mine(tmp):
    assert "NBK_JIT_OPTIONS" not in os.environ and "NBK_NO_JIT" not in os.environ
    return _masks(tmp)


def _bits(m):
    return np.unpackbits(m)[:B].astype(bool)


@pytest.mark.gpu
def test_specialised_kernel_served_every_case(mine, unfolded, generic, tmp):
    from numbotics_amd.engine import broad_spec_source
    for key in CASES + ("c2_bad",):
        assert mine[f"{key}|used"].tolist() == [sc.SPECIALISED], (key, mine[f"{key}|used"])
        assert unfolded[f"{key}|used"].tolist() == [sc.SPECIALISED], (key, unfolded[f"{key}|used"])
        assert generic[f"{key}|used"].tolist() == [sc.GENERIC], (key, generic[f"{key}|used"])
    for key in CASES:
        sm, chain = fc.case_model(key, tmp)
        assert sc.parse_spec(broad_spec_source(sm))["fc_any"] == FOLDED[key], key


@pytest.mark.gpu
@pytest.mark.parametrize("key", CASES)
def test_masks_equal_unfolded_generic_and_oracle(key, mine, unfolded, generic, tmp):
    from oracle.cpu_oracle import Oracle
    sm, chain = fc.case_model(key, tmp)
    q = _q(key, chain)
    orc = Oracle(sm)
    sample = np.unique(np.concatenate([np.arange(0, B, ORACLE_STRIDE), np.arange(B - 40, B)]))
    counts = []
    for thr in sc.THRESHOLDS:
        got, unf, gen = _bits(mine[f"{key}|{thr}"]), _bits(unfolded[f"{key}|{thr}"]), _bits(generic[f"{key}|{thr}"])
        assert np.array_equal(got, unf), f"{key} at {thr}: folded != unfolded in rows {np.flatnonzero(got != unf)[:8].tolist()}"
        assert np.array_equal(got, gen), f"{key} at {thr}: folded != generic in rows {np.flatnonzero(got != gen)[:8].tolist()}"
        ref = orc.validity(q[sample], thr, nthreads=8)
        assert np.array_equal(got[sample], ref), f"{key} at {thr}: != oracle in rows {sample[got[sample] != ref][:8].tolist()}"
        counts.append(int(got.sum()))
    print(f"{key}: colliding rows per threshold {counts} of {B}")
    assert 0 < counts[0] < B, (key, counts)


@pytest.mark.gpu
def test_bad_rows_in_every_joint_column(mine, unfolded, generic, tmp):
    from oracle.cpu_oracle import Oracle
    sm, chain = fc.case_model("c2", tmp)
    q = _q("c2_bad", chain)
    bad = _bad_rows(q.shape[1])
    waves = np.concatenate([np.arange(64 * (r // 64), 64 * (r // 64) + 64) for r in bad])
    ordinary = np.setdiff1d(waves, np.array(sorted(bad)))
    orc = Oracle(sm)
    for thr in sc.THRESHOLDS:
        got, unf, gen = _bits(mine[f"c2_bad|{thr}"]), _bits(unfolded[f"c2_bad|{thr}"]), _bits(generic[f"c2_bad|{thr}"])
        assert np.array_equal(got[waves], gen[waves]), f"at {thr}: folded != generic in rows {waves[got[waves] != gen[waves]][:8].tolist()}"
        assert np.array_equal(got, gen) and np.array_equal(got, unf), thr
        for row, (j, v) in bad.items():
            if not np.isfinite(v):
                assert got[row], (thr, row, j, v)           # NaN and +inf collide by definition
        # the ordinary rows of those waves went through the unfolded sweep: the oracle decides them the same
        ref = orc.validity(q[ordinary], thr, nthreads=8)
        assert np.array_equal(got[ordinary], ref), f"at {thr}: != oracle in rows {ordinary[got[ordinary] != ref][:8].tolist()}"
        # and every other row is c2's own
        rest = np.setdiff1d(np.arange(B), waves)
        assert np.array_equal(got[rest], _bits(mine[f"c2|{thr}"])[rest]), thr
