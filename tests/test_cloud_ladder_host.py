"""The point-cloud tests on the long-chain ladder, the part that needs no device (tests/cloud_ladder_cases.py; the GPU file is
test_gpu_cloud_ladder.py): every condition on the inputs, asserted on the references alone; what makes ``s72`` the robot it has to be
(two selection words, a caller's order that is not the device's, on both sides of shape 64); joint 31 under a selection; frames shared
and not shared by consecutive device-order shapes; and the per-shape motion bound against the oracle's FK on long paths.

Figures of the references when the cases were settled (share of the 130 configurations that collide at threshold 0 / 0.02 / -0.005
with points of radius 0.01, selection None; share of rows with a finite clearance below 0.02 and rows with a negative one, selection
arm, radius 0.01; share of the 130 sampled edges valid, connect / steer, selection arm; FREE / COLLISION / UNDECIDED of the 32 certified
edges under each of the four CONFIGS):

    k9    0.34 0.37 0.32   0.37  44   0.56 0.62   19/10/3  21/10/1  13/18/1  12/18/2
    k16   0.38 0.39 0.36   0.39  49   0.54 0.56   16/14/2  16/14/2  17/13/2  16/13/3
    k25   0.35 0.38 0.34   0.38  45   0.61 0.62   21/10/1  22/10/0  24/8/0   22/8/2
    k32d  0.38 0.40 0.38   0.40  50   0.55 0.58   19/11/2  20/11/1  20/11/1  20/11/1
    tree  0.36 0.40 0.35   0.40  47   0.59 0.59   21/8/3   22/8/2   19/13/0  18/13/1
    s72   0.35 0.36 0.34   0.36  45   0.60 0.62   16/10/6  19/10/3  21/10/1  21/10/1

s72's other selections at the three thresholds: straddle 0.18 0.21 0.15, high 0.26 0.28 0.25, low 0.34 0.36 0.33, one_high 0.17 0.19
0.15.  Every certified batch takes the +inf exit (275 .. 2108 evaluations) and, at look_ahead 0.03, the D_cap exit (305 .. 25603)."""
import ctypes as C

import numpy as np
import pytest

import cloud_ladder_cases as K
from cloud_continuous_ref import EXIT_INF, EXIT_CAP
from continuous_ref import FREE, COLLISION, UNDECIDED, DEGENERATE

SH_BOX, SH_CYLINDER = 2, 3


def mixed(ref, what):
    f = float(np.mean(ref))
    assert 0.05 <= f <= 0.70, f"{what}: {f:.3f} of the reference collides -- not a mixed case"


def cloud_of(key):
    return "sub" if key == "sub" else "arm"


def check_certified(rb, ref, config, what):
    """The conditions on a batch of certified edges, asserted on the restatement's output."""
    mode, given, la, _ = K.CONFIGS[config]
    st, exits = ref[3], ref[6]
    n_free, n_col = int((st == FREE).sum()), int((st == COLLISION).sum())
    n_rest = int((st == UNDECIDED).sum() + (st == DEGENERATE).sum())
    print(f"{what}: FREE {n_free} COLLISION {n_col} UNDECIDED {int((st == UNDECIDED).sum())} exits {exits.tolist()}")
    assert n_free >= 3 and n_col >= 3, f"{what}: {n_free} FREE, {n_col} COLLISION edges"
    assert 4 * n_rest <= st.shape[0], f"{what}: {n_rest} UNDECIDED or DEGENERATE edges of {st.shape[0]}"
    assert (st[-2:] == DEGENERATE).all()
    assert exits[EXIT_INF] >= 1, f"{what}: no item takes the +inf exit"
    if la != K.INF:
        assert exits[EXIT_CAP] >= 1, f"{what}: no item takes the D_cap exit"
    else:
        assert exits[EXIT_CAP] == 0
    if mode == "steer":
        g = K.certified_edges(rb, st.shape[0])[1]
        live = st != DEGENERATE
        assert (ref[1][live].view(np.int64) != g[live].view(np.int64)).any(), f"{what}: no edge is clipped by max_distance"


@pytest.mark.parametrize("name", K.ROBOTS)
def test_mask_and_clearance_inputs(name):
    rb = K.robot(name)
    sm = rb.sm
    sel = K.selections(rb)
    for key, shapes in sel.items():
        for r in K.RADII:
            for thr in K.THRESHOLDS:
                mixed(K.mask_ref(name, cloud_of(key), r, thr, shapes), f"{name} {key} r={r} thr={thr}")
    assert K.points(name, "arm").shape[0] <= 300 and K.points(name, "sub").shape[0] <= 300
    for key in ("arm", "sub"):
        pts = K.points(name, key)
        N = pts.shape[0]
        assert np.array_equal(pts[N - 1], pts[7]) and np.array_equal(pts[N // 2], pts[N // 2 + 50]), "the two duplicated points"
        for r in K.RADII:
            d, s, p = K.closest_ref(name, key, r, K.D_MAX[0], sel[key])
            fin = np.isfinite(d)
            assert 0.10 <= fin.mean() <= 0.90, (name, key, r, fin.mean())
            assert (d[fin] < 0).any(), "no penetrating rows in the reference"
            for d_max in K.D_MAX:
                d, s, p = K.closest_ref(name, key, r, d_max, sel[key])
                assert not np.any(p == N - 1) and not np.any(p == N // 2 + 50), "a tie goes to the smaller point index"
                assert set(s[s >= 0].tolist()) <= set(sel[key])
    if name == "s72":
        none = K.mask_ref(name, "arm", K.RADII[0], 0.0, None)
        high, low = (K.mask_ref(name, "arm", K.RADII[0], 0.0, sel[k]) for k in ("high", "low"))
        assert np.array_equal(high | low, none) and not np.array_equal(high, none) and not np.array_equal(low, none)
        assert high.mean() >= 0.05 and low.mean() >= 0.05
        for r in K.RADII:
            for d_max in K.D_MAX:
                s = K.closest_ref(name, "arm", r, d_max, sel["arm"])[1]
                assert (s >= 64).sum() >= 5, f"r={r} d_max={d_max}: the closest shape is >= 64 in {(s >= 64).sum()} rows"


def test_points_inside_boxes_and_cylinders():
    """Over the ladder, the rows with a negative clearance whose closest shape is a box, and those whose closest shape is a cylinder:
    at least three each (the two kinds whose cores have volume: a point inside one sends the distance to EPA).  Counted when the cases
    were settled (radius 0.01, selection arm + selection sub): box 130, cylinder 75."""
    count = {SH_BOX: 0, SH_CYLINDER: 0}
    for name in K.ROBOTS:
        rb = K.robot(name)
        for key in ("arm", "sub"):
            d, s, p = K.closest_ref(name, key, K.RADII[0], K.D_MAX[1], K.selections(rb)[key])
            kinds = rb.sm.rshape_type[s[d < 0]]
            for t in count:
                count[t] += int((kinds == t).sum())
    print("negative rows by the closest shape's type:", count)
    assert count[SH_BOX] >= 3 and count[SH_CYLINDER] >= 3, count


@pytest.mark.parametrize("name", K.ROBOTS)
def test_edge_inputs(name):
    """Sampled edges: between 15 % and 85 % valid (both verdicts well represented among 130), and in steer mode some edge is cut at
    max_distance.  Certified edges: the conditions of check_certified for the four CONFIGS, and for s72's high and straddle."""
    rb = K.robot(name)
    sel = K.selections(rb)
    keys = ["arm"] + (["straddle", "high"] if name == "s72" else [])
    for key in keys:
        for mode in ("connect", "steer"):
            valid, end, ns = K.sampled_ref(name, "arm", K.RADII[0], 0.0, mode, False, sel[key])
            print(f"{name} {key} {mode}: {valid.mean():.2f} valid, {ns.min()}..{ns.max()} samples")
            assert 0.15 <= valid.mean() <= 0.85, (name, key, mode, valid.mean())
            assert ns.max() >= 8
    s, g = K.edges(rb)
    assert (K.sampled_ref(name, "arm", K.RADII[0], 0.0, "steer", False, sel["arm"])[1].view(np.int64) != g.view(np.int64)).any()
    for config, (mode, given, la, key) in enumerate(K.CONFIGS):
        ref = K.certified_ref(name, cloud_of(key), config, sel[key])
        check_certified(rb, ref, config, f"{name} {mode} dist={'given' if given else 'None'} look_ahead={la} shapes={key}")
    ref = K.certified_ref(name, "arm", 0, sel["arm"])
    assert ((ref[3] == UNDECIDED) & (ref[2] > 0.0)).any(), "no edge is stopped on its way (by a point at an interior point of an edge)"
    if name == "s72":
        for key in ("high", "straddle"):
            check_certified(rb, K.certified_ref(name, "arm", 0, sel[key]), 0, f"s72 {key}")


def test_accumulate_inputs_on_k16():
    """k16's own scene and its cloud each stop edges the other lets through, under the sampled and under the certified check."""
    for mode in ("connect", "steer"):
        own, only, both = K.sampled_accumulate_ref(mode)
        assert np.array_equal(both[0], own[0] & only[0])
        assert (~own[0] & only[0]).sum() >= 3 and (own[0] & ~only[0]).sum() >= 3 and both[0].sum() >= 3
    for mode, la in (("connect", 0.03), ("steer", K.INF)):
        own, only, both = K.certified_accumulate_ref(mode, la)
        assert ((own[3] != FREE) & (only[3] == FREE)).sum() >= 3 and ((own[3] == FREE) & (only[3] != FREE)).sum() >= 3
        assert (both[3] == FREE).sum() >= 3


def test_the_second_cloud_of_k32d_differs():
    """The graph test swaps k32d's cloud for another of as many points in the same box."""
    shapes = K.selections(K.robot("k32d"))["arm"]
    assert K.points("k32d", "arm", 0).shape == K.points("k32d", "arm", 1).shape
    first, other = (K.mask_ref("k32d", "arm", K.RADII[0], 0.0, shapes, seed_shift=k) for k in (0, 1))
    assert (first != other).sum() >= 3
    mixed(other, "k32d, the second cloud")
    lo, hi = K.bounds("k32d")
    for k in (0, 1):
        p = K.points("k32d", "arm", k)
        assert (p > np.array(lo)).all() and (p < np.array(hi)).all()


def test_s72_needs_two_words_and_two_orders():
    from numbotics_amd import _lib
    from numbotics_amd.engine import model_desc
    rb = K.robot("s72")
    sm = rb.sm
    S = sm.n_rshapes
    assert 65 <= S <= 96 and sm.kin.n_q == 32 and sm.kin.n_joints == 32
    per_link = np.bincount(sm.rshape_link, minlength=len(sm.links))
    assert per_link.max() == 3 and (per_link == 3).sum() >= 8 and (per_link[1:] == 0).sum() >= 3, per_link
    # accepted: the descriptor passes the host's checks, and its LDS broadphase layout is within the limit of nbk_model_create
    d, keep = model_desc(sm)
    s, g = K.edges(rb)
    mu = np.empty((2, S))
    assert _lib.load().nbk_edge_shape_motion_bounds_host(C.byref(d), s.ctypes.data, g.ctypes.data, 2, mu.ctypes.data) == 0
    assert K.L.frame_slots(sm.kin) == 0 and K.lds_broad_bytes(sm) <= K.L.LDS_MAX, K.lds_broad_bytes(sm)
    # the same formula puts the largest serial chain without pairs at 104 shapes (n_q <= 3), 102 at n_q = 9: never a third word
    room = lambda n_q: (K.L.LDS_MAX - 2048 - K.L.ROW * n_q) // (3 * K.L.ROW)
    assert room(3) == 104 and room(9) == 102 and room(1) < 128
    order = K.device_order(sm)
    moved = np.flatnonzero(order != np.arange(S))
    assert (moved >= 64).any() and (moved < 64).any(), moved
    # a selection's words differ between the two orders; the device's words of high (and of arm) hold set bits on both sides of 64,
    # so the certified kernel's count of selected shapes crosses from word 0 into word 1
    for key in ("high", "straddle", "sub", "arm"):
        chosen = np.isin(order, K.selections(rb)[key])              # device position i is selected
        user = np.isin(np.arange(S), K.selections(rb)[key])
        assert not np.array_equal(chosen, user), key
        if key == "high":
            assert not np.array_equal(chosen[:64], user[:64]) and not np.array_equal(chosen[64:], user[64:]), key
        if key in ("high", "arm"):
            assert chosen[:64].any() and chosen[64:].any(), f"{key}: both words hold a set bit in device order"


def test_joint_31_is_on_a_selected_path():
    """rs_mask bit 31: under every selection of k32d, and on s72 under None, arm and high (whose bits lie in the second word)."""
    for name, keys in (("k32d", ("all", "arm", "sub")), ("s72", ("all", "arm", "high"))):
        rb = K.robot(name)
        sm = rb.sm
        assert sm.kin.n_joints == 32
        for key in keys:
            shapes = K.selections(rb)[key]
            shapes = range(sm.n_rshapes) if shapes is None else shapes
            paths = [sm.kin.frames[sm.links[sm.rshape_link[s]]._name].path.tolist() for s in shapes]
            assert any(31 in p for p in paths), (name, key)


@pytest.mark.parametrize("name", K.ROBOTS)
def test_consecutive_shapes_share_a_frame_and_do_not(name):
    """In device order, under None and under arm: a lane keeps its frame across the first kind of neighbours and replays FK across
    the second; with empty links in between the replayed frame is not the next joint's."""
    rb = K.robot(name)
    sm = rb.sm
    fr = sm.rshape_frame[K.device_order(sm)]
    assert (np.diff(fr) >= 0).all()
    for key in ("all", "arm"):
        f = fr if key == "all" else fr[fr >= 0]
        same, other = int((np.diff(f) == 0).sum()), int((np.diff(f) > 0).sum())
        assert same >= 1 and other >= 1, (name, key, same, other)
    assert (np.diff(fr) > 1).any(), "no empty link between two links that carry shapes"
    if name == "tree":
        par = np.asarray(sm.kin.joint_parent)
        assert any(par[b] != a for a, b in zip(fr[:-1], fr[1:]) if b > a >= 0), "device order follows one path"


@pytest.mark.parametrize("name", K.ROBOTS)
def test_shape_motion_bound_holds_on_long_paths(name):
    """mu[e, s] |t - t'| bounds how far a point of shape s moves between q(t) and q(t') on edge e: checked on the shape's centre
    and on the six points one bounding radius from it along the shape's axes, under the oracle's FK, for 50 pairs (t, t') on each of
    16 edges.  The allowance of 1e-9 relative + 1e-12 covers the rounding of two FK chains of 32 joints (some 1e-14)."""
    from numbotics_amd.engine import edge_shape_motion_bounds
    from oracle.cpu_oracle import Oracle
    rb = K.robot(name)
    sm = rb.sm
    S = sm.n_rshapes
    s, g = K.edges(rb)
    s, g = s[:16], g[:16]
    mu = edge_shape_motion_bounds(sm, s, g)
    assert mu.shape == (16, S) and (mu >= 0.0).all() and (mu[:, sm.rshape_frame >= 0] > 0.0).all() and (mu[:, sm.rshape_frame < 0] == 0.0).all()
    rng = np.random.default_rng(3)
    t = rng.uniform(0.0, 1.0, (16, 50, 2))
    t[:, 0] = (0.0, 1.0)                                           # the whole edge among them
    rad = K.bound_radii(sm, range(S))
    local = np.zeros((7, 4))
    local[:, 3] = 1.0
    for a in range(3):
        local[1 + 2 * a, a], local[2 + 2 * a, a] = 1.0, -1.0
    orc = Oracle(sm.kin)
    worst = 0.0
    for e in range(16):
        tt = t[e].reshape(-1)
        q = (1.0 - tt)[:, None] * s[e] + tt[:, None] * g[e]
        poses = {}
        for x in range(S):
            link = sm.links[sm.rshape_link[x]]._name
            if link not in poses:
                poses[link] = orc.fk(q, link) @ np.linalg.inv(np.asarray(sm.kin.frames[link].local, dtype=np.float64))
            P = local.copy()
            P[:, :3] *= rad[x]
            w = np.einsum("bij,jk,pk->bpi", poses[link], K._T44(sm.rshape_local[x]), P)[:, :, :3].reshape(50, 2, 7, 3)
            moved = np.linalg.norm(w[:, 0] - w[:, 1], axis=2).max(axis=1)
            bound = mu[e, x] * np.abs(t[e, :, 0] - t[e, :, 1])
            assert (moved <= bound * (1.0 + 1e-9) + 1e-12).all(), f"{name} edge {e} shape {x}: moved {moved.max()} against {bound.max()}"
            worst = max(worst, float((moved / np.maximum(bound, 1e-300)).max()))
    print(f"{name}: the largest displacement is {worst:.3f} of its bound")
    assert worst > 0.05, "the bound is never approached: the sample points do not test it"
