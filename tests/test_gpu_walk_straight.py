"""The straight-line GJK walk step of the narrowphase (gjkb_step_sl: values computed whatever the case and selected, where
gjkb_step_k branches) against the oracle, bit for bit, on the walks a selected-instead-of-branched value would break first: the
near-tangent ones.  For one cylinder-cylinder, one box-cylinder and one box-box pair of c2 a joint angle is bisected to the
free / colliding boundary with the oracle and 2 001 angles in steps of 1e-10 rad are swept across it, at thresholds 0, 1e-6 and
0.01, on the default (Bullet margins: inflated walks) and on the sharp shapes.  Then one batch of 2^16 random q per scene."""
import numpy as np
import pytest

from oracle.cpu_oracle import Oracle
from numbotics_amd.robots.model import SH_BOX, SH_CYLINDER
from numbotics_amd.scenes import build_scene, sample_q

THRESHOLDS = (0.0, 1e-6, 0.01)
CLASSES = {"cylinder-cylinder": (SH_CYLINDER, SH_CYLINDER), "box-cylinder": (SH_BOX, SH_CYLINDER), "box-box": (SH_BOX, SH_BOX)}
CLEAR = 0.02          # every other pair stays this far away at both ends of the bisection: the chosen pair decides the mask
N_SWEEP = 2001
STEP = 1e-10


def pair_kinds(sm):
    """(P, 2) shape types of every pair, sorted within the pair."""
    S = sm.n_rshapes
    ta = sm.rshape_type[sm.pair_a]
    tb = np.where(sm.pair_b < S, sm.rshape_type[np.minimum(sm.pair_b, S - 1)], sm.wshape_type[np.maximum(sm.pair_b - S, 0)])
    return np.sort(np.stack([ta, tb], axis=1), axis=1)


def find_boundary(orc, sm, chain, kinds, thr, seed=5):
    """-> (q at the boundary, colliding side; joint; pair): the first sampled configuration where a pair of `kinds` collides
    alone and a move of one joint frees it with every other pair still clear, bisected with the oracle at threshold `thr`."""
    want = np.sort(np.asarray(kinds))
    cls = np.nonzero((pair_kinds(sm) == want).all(axis=1))[0]
    base = sample_q(chain, 4000, seed=seed)
    D = orc.pair_distances(base)
    for p in cls:
        others = np.delete(np.arange(sm.n_pairs), p)
        for i in np.nonzero((D[:, p] < 0.0) & (D[:, others].min(axis=1) > CLEAR))[0][:20]:
            for j in range(chain.dof):
                for step in (0.05, -0.05, 0.2, -0.2, 0.6, -0.6):
                    lo, hi = base[i].copy(), base[i].copy()
                    lo[j] += step
                    dl = orc.pair_distances(lo[None])[0]
                    if not (dl[p] > 2.0 * max(thr, 0.0) + 1e-3 and dl[others].min() > CLEAR):
                        continue
                    if orc.validity(lo[None], thr)[0] or not orc.validity(hi[None], thr)[0]:
                        continue
                    for _ in range(70):                      # down to the last bits of the angle
                        mid = 0.5 * (lo + hi)
                        if orc.validity(mid[None], thr)[0]:
                            hi = mid
                        else:
                            lo = mid
                    return hi, j, int(p)
    return None


def sweep(hi, j):
    q = np.tile(hi, (N_SWEEP, 1))
    q[:, j] = hi[j] + (np.arange(N_SWEEP) - N_SWEEP // 2) * STEP
    return q


@pytest.mark.gpu
@pytest.mark.parametrize("margins", [True, False], ids=["bullet", "sharp"])
@pytest.mark.parametrize("cls", list(CLASSES))
def test_near_tangent_walks_match_the_oracle(fresh_world, cls, margins):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    arm, chain, obs = build_scene("c2", bullet_margins=margins)
    sm = arm.scene_model()
    orc = Oracle(sm)
    for thr in THRESHOLDS:
        found = find_boundary(orc, sm, chain, CLASSES[cls], thr)
        assert found is not None, (cls, margins, thr, "no boundary found")
        hi, j, p = found
        q = sweep(hi, j)
        ref = orc.validity(q, thr, nthreads=8)
        assert ref.any() and not ref.all(), (cls, margins, thr, "the sweep does not cross the boundary")
        got = np.asarray(arm.in_collision(q, thr))
        print(f"{cls} {'bullet' if margins else 'sharp'} thr {thr:g}: pair {p} joint {j} colliding {int(ref.sum())} of {N_SWEEP}, "
              f"mismatches {int((got != ref).sum())}")
        assert np.array_equal(got, ref), (cls, margins, thr, int((got != ref).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["c2", "c3", "c2m", "c5m"])
def test_random_batch_matches_the_oracle(fresh_world, scene):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    arm, chain, obs = build_scene(scene)
    q = sample_q(chain, 1 << 16, seed=21)
    got = np.asarray(arm.in_collision(q, 0.0))
    ref = Oracle(arm.scene_model()).validity(q[::16], 0.0, nthreads=8)
    assert np.array_equal(got[::16], ref), (scene, int((got[::16] != ref).sum()))
