"""The four point-cloud entry points (nbk_cloud_validity_batch, nbk_cloud_clearance_batch, nbk_edge_cloud_validity_batch,
nbk_edge_cloud_continuous_batch) on the long-chain ladder and on a robot of 72 shapes (tests/cloud_ladder_cases.py), bit for bit
against the CPU oracle with the cloud's points as sphere world shapes (tests/cloud_cases.py) and against the restatement of the
certified loop (tests/cloud_continuous_ref.py).  Needs a real MI355X.

What only these robots reach: q rows of 9, 16, 25 and 32 values through cloud_stage_q and CloudEdgeLane::distance; bit 31 of a
shape's joint mask; frames kept across consecutive shapes of one link and replayed across empty links and across the branches of a
tree; a second selection word, and on s72 -- whose shapes the descriptor lists in a shuffled order -- selection bits, reported
shapes and motion-bound columns that differ between the caller's order and the device's.

The conditions on the inputs (mixed verdicts, both exits, clipped edges, points inside boxes and cylinders, ...) are asserted on
the references in test_cloud_ladder_host.py, which runs without a device; the references are computed once per process
(cloud_ladder_cases caches them) and shared by the tests here.

CPU time of the references when the cases were settled, per robot (the two clouds and the masks of every selection, radius and
threshold / clearances / sampled edges / the four certified CONFIGS): k9 0.6 / 0.1 / 0.1 / 1.4 s, k16 0.8 / 0.1 / 0.1 / 0.1 s, k25
1.1 / 0.1 / 0.1 / 0.3 s, k32d 2.3 / 0.2 / 0.2 / 0.8 s, tree 1.5 / 0.2 / 0.2 / 0.3 s, s72 4.3 / 0.4 / 0.5 / 0.9 s; the 65-edge batch
of the first config about doubles the last figure.  So every robot keeps E_CASE = 34 certified edges."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_parity import assert_bitwise, torch_cuda      # noqa: F401  (fixture)
from cloud_cases import pack_bits
import cloud_ladder_cases as K
from cloud_ladder_cases import INF

R = K.RADII[0]


@functools.lru_cache(maxsize=None)
def device(name):
    """The robot's descriptor on the device, created once per process."""
    from numbotics_amd.engine import DeviceModel
    return DeviceModel(K.robot(name).sm)


def cloud_of(key):
    return "sub" if key == "sub" else "arm"


def selection_keys(name):
    return ("all", "arm", "sub") + (("straddle", "high", "low", "one_high") if name == "s72" else ())


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_certified(dev, ref, what, n=None):
    v, end, tf, st = (_host(x) for x in dev)
    rv, rend, rtf, rst = (a if n is None else a[:n] for a in ref[:4])
    assert np.array_equal(v.astype(bool), rv), f"{what}: valid differs on {np.nonzero(v.astype(bool) != rv)[0][:10]}"
    assert np.array_equal(st, rst), f"{what}: status differs on {np.nonzero(st != rst)[0][:10]}: {st[st != rst][:10]} vs {rst[st != rst][:10]}"
    assert np.array_equal(_bits(tf), _bits(rtf)), f"{what}: t_free differs on {np.nonzero(_bits(tf) != _bits(rtf))[0][:10]}"
    assert np.array_equal(_bits(end), _bits(rend)), f"{what}: end differs"


def _same_sampled(got, ref, what, n=None):
    valid, end, ns = (_host(x) for x in got)
    ref = ref if n is None else tuple(a[:n] for a in ref)
    assert np.array_equal(valid.astype(bool), ref[0]), f"{what}: valid differs at {np.flatnonzero(valid.astype(bool) != ref[0])[:8]}"
    assert_bitwise(end, ref[1], f"{what}: end")
    assert ns.dtype == np.int32 and np.array_equal(ns, ref[2]), f"{what}: n_samples"


# ---- 1. masks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.ROBOTS)
def test_masks(name, torch_cuda):
    from numbotics_amd.physics import PointCloud
    rb, dev = K.robot(name), device(name)
    sel = K.selections(rb)
    for which in ("arm", "sub"):
        pts = K.points(name, which)
        for r in K.RADII:
            cloud = PointCloud(pts.copy(), r)
            assert cloud.status() == 0 and cloud.n == pts.shape[0]
            for key in (k for k in selection_keys(name) if cloud_of(k) == which):
                for thr in K.THRESHOLDS:
                    ref = K.mask_ref(name, which, r, thr, sel[key])
                    what = f"{name} {key} r={r} thr={thr}"
                    for B in K.BATCHES:
                        m = dev.cloud_validity(cloud, rb.q[:B], thr, shapes=sel[key])
                        assert m.dtype == bool and np.array_equal(m, ref[:B]), f"{what} B={B}: bytes differ at {np.flatnonzero(m != ref[:B])[:8]}"
                        w = dev.cloud_validity(cloud, rb.q[:B], thr, packed=True, shapes=sel[key])
                        assert np.array_equal(w, pack_bits(ref[:B])), f"{what} B={B}: packed words differ"


def test_s72_high_and_low_accumulate_to_every_shape(torch_cuda):
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    rb, dev = K.robot("s72"), device("s72")
    sel = K.selections(rb)
    cloud = PointCloud(K.points("s72").copy(), R)
    qt = torch.from_numpy(rb.q).cuda()
    for thr in K.THRESHOLDS:
        none, high, low = (K.mask_ref("s72", "arm", R, thr, sel[k]) for k in ("all", "high", "low"))
        assert np.array_equal(high | low, none) and not np.array_equal(high, none)
        for B in K.BATCHES:
            mask = dev.cloud_validity(cloud, qt[:B], thr, shapes=sel["high"])
            assert np.array_equal(mask.cpu().numpy(), high[:B]), f"high alone, thr={thr} B={B}"
            got = dev.cloud_validity(cloud, qt[:B], thr, shapes=sel["low"], out=mask)
            assert got is mask and np.array_equal(mask.cpu().numpy(), none[:B]), f"high, then low into it: thr={thr} B={B}"
            words = dev.cloud_validity(cloud, qt[:B], thr, packed=True, shapes=sel["low"])
            dev.cloud_validity(cloud, qt[:B], thr, packed=True, shapes=sel["high"], out=words)
            assert np.array_equal(words.cpu().numpy(), pack_bits(none[:B])), f"low, then high into it, packed: thr={thr} B={B}"


# ---- 2. clearance -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.ROBOTS)
def test_clearance(name, torch_cuda):
    from numbotics_amd.physics import PointCloud
    rb, dev = K.robot(name), device(name)
    sel = K.selections(rb)
    keys = ("arm", "sub", "all") + (("high", "straddle") if name == "s72" else ())
    for which in ("arm", "sub"):
        for r in K.RADII:
            cloud = PointCloud(K.points(name, which).copy(), r)
            for key in (k for k in keys if cloud_of(k) == which):
                for d_max in K.D_MAX:
                    dr, sr, pr = K.closest_ref(name, which, r, d_max, sel[key])
                    if key == "sub":
                        assert set(sr[sr >= 0].tolist()) <= set(sel["sub"]) and (sr >= 0).any()
                    for B in (65, 130):
                        d, s, p = dev.cloud_clearance(cloud, rb.q[:B], d_max, shapes=sel[key])
                        what = f"{name} {key} r={r} d_max={d_max} B={B}"
                        assert_bitwise(d, dr[:B], f"{what}: distance")
                        assert np.array_equal(s, sr[:B]), f"{what}: shape differs at {np.flatnonzero(s != sr[:B])[:8]}: {s[s != sr[:B]][:8]} vs {sr[:B][s != sr[:B]][:8]}"
                        assert np.array_equal(p, pr[:B]), f"{what}: point"


# ---- 3. sampled edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.ROBOTS)
def test_sampled_edges(name, torch_cuda):
    from numbotics_amd.physics import PointCloud
    rb, dev = K.robot(name), device(name)
    sel = K.selections(rb)
    s, g = K.edges(rb)
    given = K.given_dist(s, g)
    cloud = PointCloud(K.points(name).copy(), R)
    keys = ("arm",) + (("straddle", "high") if name == "s72" else ())
    for key in keys:
        for mode in ("connect", "steer"):
            for dist in ((None, given) if key == "arm" else (None,)):
                ref = K.sampled_ref(name, "arm", R, 0.0, mode, dist is not None, sel[key])
                for E in K.E_SIZES:
                    got = dev.cloud_edge_validity(cloud, s[:E], g[:E], K.RESOLUTION, K.MAXD, mode=mode, dist=None if dist is None else dist[:E],
                                                  shapes=sel[key])
                    assert got[0].dtype == bool
                    _same_sampled(got, ref, f"{name} {key} {mode} dist={'given' if dist is not None else 'None'} E={E}", E)


def test_sampled_edges_accumulate_on_k16(torch_cuda):
    """edge_validity of k16's own scene, then the cloud's verdicts ANDed into the same ``valid`` = the oracle on the descriptor that
    holds both."""
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    rb, dev = K.robot("k16"), device("k16")
    shapes = K.selections(rb)["arm"]
    s, g = K.edges(rb)
    st, gt = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
    cloud = PointCloud(K.points("k16").copy(), R)
    for mode in ("connect", "steer"):
        own, only, both = K.sampled_accumulate_ref(mode)
        assert np.array_equal(both[0], own[0] & only[0])
        assert (~own[0] & only[0]).sum() >= 3 and (own[0] & ~only[0]).sum() >= 3 and both[0].sum() >= 3, "each side must block edges of its own"
        valid, end, ns = dev.edge_validity(st, gt, K.RESOLUTION, K.MAXD, mode=mode)
        assert np.array_equal(valid.cpu().numpy().astype(bool), own[0])
        got = dev.cloud_edge_validity(cloud, st, gt, K.RESOLUTION, K.MAXD, mode=mode, shapes=shapes, out=valid)
        assert got[0] is valid
        _same_sampled((valid, got[1], got[2]), both, f"accumulated {mode}")
        assert_bitwise(end.cpu().numpy(), got[1].cpu().numpy(), "the end states of the two calls")


# ---- 4. certified edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", range(len(K.CONFIGS)), ids=[f"{m}-{'dist' if d else 'nodist'}-{la}-{k}" for m, d, la, k in K.CONFIGS])
@pytest.mark.parametrize("name", K.ROBOTS)
def test_certified_edges(name, config, torch_cuda):
    from numbotics_amd.physics import PointCloud
    rb, dev = K.robot(name), device(name)
    mode, given, la, key = K.CONFIGS[config]
    shapes = K.selections(rb)[key]
    cloud = PointCloud(K.points(name, cloud_of(key)).copy(), R)
    maxd = K.STEER_MAXD if mode == "steer" else 10.0
    # E_CASE edges; under the first config also 1, 63 and 65 of the batch of 63 edges and two degenerate ones
    batches = [(None, (K.E_CASE[name],))] + ([(65, (1, 63, 65))] if config == 0 else [])
    for n, sizes in batches:
        s, g = K.certified_edges(rb, n)
        dist = K.given_dist(s, g) if given else None
        ref = K.certified_ref(name, cloud_of(key), config, shapes, n)
        assert (ref[3][-2:] == 3).all() and (ref[3][:-2] != 3).all()
        for E in sizes:
            got = dev.cloud_edge_continuous(cloud, s[:E], g[:E], maxd, mode=mode, look_ahead=la, dist=None if dist is None else dist[:E],
                                            shapes=shapes)
            assert got[0].dtype == bool and got[3].dtype == np.int32
            _same_certified(got, ref, f"{name} {mode} dist={'given' if given else 'None'} look_ahead={la} shapes={key} E={E}", E)


@pytest.mark.parametrize("key", ["high", "straddle"])
def test_certified_edges_across_the_selection_words_of_s72(key, torch_cuda):
    """The grid's y dimension counts the selected shapes in device order: under ``high`` from word 0 into word 1."""
    from numbotics_amd.physics import PointCloud
    rb, dev = K.robot("s72"), device("s72")
    shapes = K.selections(rb)[key]
    cloud = PointCloud(K.points("s72").copy(), R)
    s, g = K.certified_edges(rb)
    ref = K.certified_ref("s72", "arm", 0, shapes)
    got = dev.cloud_edge_continuous(cloud, s, g, 10.0, look_ahead=K.CONFIGS[0][2], shapes=shapes)
    _same_certified(got, ref, f"s72 {key}")


def test_certified_edges_accumulate_on_k16(torch_cuda):
    """edge_continuous of k16's own scene, then the cloud's items reduced into its result = one certified call over both."""
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    from continuous_ref import FREE, DEGENERATE
    rb, dev = K.robot("k16"), device("k16")
    shapes = K.selections(rb)["arm"]
    s, g = K.certified_edges(rb)
    st_, gt_ = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
    cloud = PointCloud(K.points("k16").copy(), R)
    for mode, la in (("connect", 0.03), ("steer", INF)):
        maxd = K.STEER_MAXD if mode == "steer" else 10.0
        own, only, both = K.certified_accumulate_ref(mode, la)
        assert ((own[3] != FREE) & (only[3] == FREE)).sum() >= 3 and ((own[3] == FREE) & (only[3] != FREE)).sum() >= 3, \
            "each side must stop edges of its own"
        assert (both[3] == FREE).sum() >= 3
        valid, end, t_free, status = dev.edge_continuous(st_, gt_, maxd, mode=mode)
        _same_certified((valid, end, t_free, status), own, f"scene alone {mode}")
        t_scene = t_free.clone()
        got = dev.cloud_edge_continuous(cloud, st_, gt_, maxd, mode=mode, look_ahead=la, shapes=shapes, out=(valid, t_free, status))
        assert got[0] is valid and got[2] is t_free and got[3] is status
        _same_certified(got, both, f"accumulated {mode} look_ahead={la}")
        assert np.array_equal(_bits(got[1].cpu().numpy()), _bits(end.cpu().numpy())), "the end states of the two calls"
        live = both[3] != DEGENERATE
        assert (t_free.cpu().numpy()[live] <= t_scene.cpu().numpy()[live]).all(), "an edge's stop point only ever moves down"


# ---- 5. capture -------------------------------------------------------------------------------------------------------------------
def test_update_and_four_queries_in_one_graph_on_k32d(torch_cuda):
    """A cloud update and the four queries captured on one stream with a static points tensor; the replay after the tensor's points
    were swapped on the device equals the direct calls and the references of the second cloud."""
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    name = "k32d"
    rb, dev = K.robot(name), device(name)
    shapes = K.selections(rb)["arm"]
    first, other = K.points(name, "arm", 0), K.points(name, "arm", 1)
    assert first.shape == other.shape
    s, g = K.edges(rb)
    cs, cg = K.certified_edges(rb)
    qt = torch.from_numpy(rb.q).cuda()
    st, gt, cst, cgt = (torch.from_numpy(a).cuda() for a in (s, g, cs, cg))
    Pt = torch.from_numpy(first.copy()).cuda()
    ws = torch.empty((dev.cloud_edge_workspace_bytes(s.shape[0]),), dtype=torch.uint8, device="cuda")
    cloud = PointCloud(Pt, R, bounds=K.bounds(name))
    la = K.CONFIGS[0][2]

    def run():
        mask = dev.cloud_validity(cloud, qt, 0.0, shapes=shapes)
        clr = dev.cloud_clearance(cloud, qt, K.D_MAX[0], shapes=shapes)
        smp = dev.cloud_edge_validity(cloud, st, gt, K.RESOLUTION, K.MAXD, shapes=shapes, workspace=ws)
        cer = dev.cloud_edge_continuous(cloud, cst, cgt, 10.0, look_ahead=la, shapes=shapes)
        return mask, clr, smp, cer
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                      # warm-up outside the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            cloud.update(Pt)
            mask, clr, smp, cer = run()
    torch.cuda.current_stream().wait_stream(side)
    Pt.copy_(torch.from_numpy(other.copy()).cuda())
    graph.replay()
    torch.cuda.synchronize()
    replayed = [_host(x).copy() for x in (mask, *clr, *smp, *cer)]
    cloud.update(Pt)
    direct = run()
    torch.cuda.synchronize()
    direct = [_host(x) for x in (direct[0], *direct[1], *direct[2], *direct[3])]
    for k, (a, b) in enumerate(zip(replayed, direct)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"output {k} of the replay differs from the direct call"
    ref_first = K.mask_ref(name, "arm", R, 0.0, shapes)
    ref = K.mask_ref(name, "arm", R, 0.0, shapes, seed_shift=1)
    assert (ref != ref_first).sum() >= 3, "the two clouds must differ in their verdicts"
    assert np.array_equal(replayed[0].astype(bool), ref)
    dr, sr, pr = K.closest_ref(name, "arm", R, K.D_MAX[0], shapes, seed_shift=1)
    assert_bitwise(replayed[1], dr, "replayed clearance")
    assert np.array_equal(replayed[2], sr) and np.array_equal(replayed[3], pr)
    _same_sampled(replayed[4:7], K.sampled_ref(name, "arm", R, 0.0, "connect", False, shapes, seed_shift=1), "replayed sampled edges")
    _same_certified(replayed[7:11], K.certified_ref(name, "arm", 0, shapes, seed_shift=1), "replayed certified edges")
    assert cloud.status() == 0
