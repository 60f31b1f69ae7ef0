"""Sampled straight-line edges against a point cloud on the device (nbk_edge_cloud_validity_batch, DeviceModel.cloud_edge_validity,
ConnectorParams(cloud=...)): ``valid`` equal, ``end`` and ``n_samples`` bit-identical to the CPU oracle's edge_validity on the same
robot with the cloud's points as sphere world shapes (tests/cloud_cases.py).  Needs a real MI355X.

Every mixed case asserts on the REFERENCE, before comparing, that between 25 % and 85 % of its edges are valid."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.cpu_oracle import Oracle, edge_samples
from numbotics_amd.scenes import build_scene, sample_q
from test_gpu_parity import assert_bitwise, torch_cuda      # noqa: F401  (fixture)
from cloud_cases import scan, cloud_model, cloud_mask
import long_chain_cases as lc

MAXD = 0.25
SETS = {"a": dict(length=0.3, resolution=0.05, thr=0.0), "b": dict(length=0.6, resolution=0.02, thr=0.02)}
CLOUDS = ((65, 0.02), (300, 0.01))                      # (N, radius); the points are scan(N, seed=N)
MODES = ("connect", "steer")
ROBOTS = [("c1", True), ("c2m", False), ("k9", True)]
NT = 8


def edges(q, E, seed, length):
    rng = np.random.default_rng(seed); s = q[:E].copy()
    d = rng.standard_normal(s.shape); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return s, s + d * rng.uniform(0.02, length, (E, 1))


def _robot(name, margins, tmp):
    """-> (arm, things to keep alive, q (256, dof))."""
    if name == "k9":
        arm, chain, obs = lc.case("k9", tmp)
        return arm, (chain, obs), lc.sample(chain, 256, 3)
    arm, chain, obs = build_scene(name, bullet_margins=margins)
    return arm, (chain, obs), sample_q(chain, 256, seed=3)


@functools.lru_cache(maxsize=None)
def _pts(n, seed=None):
    p = np.ascontiguousarray(scan(n, seed=n if seed is None else seed))
    return p


def _mixed(valid, what):
    f = float(np.mean(valid))
    assert 0.25 <= f <= 0.85, f"{what}: {f:.3f} of the reference's edges are valid -- not a mixed case"


def _ref(sm, pts, r, shapes, s, g, resolution, mode, thr, dist=None, keep_scene=False):
    """The oracle's (valid, end, n_samples) of the edges against the cloud (with sm's own scene: keep_scene)."""
    return Oracle(cloud_model(sm, pts, r, shapes, keep_scene=keep_scene)).edge_validity(s, g, resolution, MAXD, mode=mode, threshold=thr,
                                                                                       dist=dist, nthreads=NT)


def _compare(got, ref, what):
    valid, end, ns = got
    assert valid.dtype == bool and np.array_equal(valid, ref[0]), f"{what}: valid differs at {np.flatnonzero(valid != ref[0])[:8]}"
    assert_bitwise(end, ref[1], f"{what}: end")
    assert ns.dtype == np.int32 and np.array_equal(ns, ref[2]), f"{what}: n_samples"


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,margins", ROBOTS, ids=[f"{n}-{'bullet' if m else 'sharp'}" for n, m in ROBOTS])
def test_cloud_edges_parity(fresh_world, tmp_path, name, margins, torch_cuda):
    from numbotics_amd.physics import PointCloud
    arm, keep, q = _robot(name, margins, tmp_path)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    shapes = list(range(1, sm.n_rshapes))                       # the base shape stands on the table
    sizes = (1, 65, 200) if name == "c1" else (200,)
    for N, r in CLOUDS:
        cloud = PointCloud(_pts(N), r)
        for key, p in SETS.items():
            s, g = edges(q, 200, 7, p["length"])
            given = 1.1 * np.linalg.norm(g - s, axis=1)
            for mode in MODES:
                for dist in (None, given):
                    what = f"{name} N={N} set {key} {mode} dist={'given' if dist is not None else 'None'}"
                    ref = _ref(sm, _pts(N), r, shapes, s, g, p["resolution"], mode, p["thr"], dist)
                    _mixed(ref[0], what)
                    for E in sizes:
                        got = dev.cloud_edge_validity(cloud, s[:E], g[:E], p["resolution"], MAXD, mode=mode, threshold=p["thr"],
                                                      dist=None if dist is None else dist[:E], shapes=shapes)
                        _compare(got, tuple(a[:E] for a in ref), f"{what} E={E}")


# ---- 2. the flat mapping ---------------------------------------------------------------------------------------------------------
def _filler(q0, count, resolution):
    """An edge from q0 of exactly `count` samples in connect mode (count >= 2): n = ceil(d / resolution) = count - 1."""
    d = np.zeros_like(q0); d[-1] = 1.0
    return q0, q0 + d * ((count - 1.5) * resolution)


def test_cloud_edges_flat_mapping(fresh_world, torch_cuda):
    from numbotics_amd.physics import PointCloud
    arm, keep, q = _robot("c1", True, None)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    shapes = list(range(1, sm.n_rshapes))
    N, r = CLOUDS[1]
    pts = _pts(N)
    cloud = PointCloud(pts, r)
    res, thr = SETS["a"]["resolution"], SETS["a"]["thr"]
    s0, g0 = edges(q, 40, 11, 0.3)
    base_total = int(_ref(sm, pts, r, shapes, s0, g0, res, "connect", thr)[2].sum())
    fill = (-base_total) % 64
    fill += 64 if fill < 3 else 0
    # sample totals of exactly a multiple of 64, one more and one fewer
    for extra in (0, 1, -1):
        fs, fg = _filler(q[200], fill + extra, res)
        s, g = np.vstack((s0, fs[None])), np.vstack((g0, fg[None]))
        ref = _ref(sm, pts, r, shapes, s, g, res, "connect", thr)
        assert int(ref[2].sum()) % 64 == extra % 64 and ref[2][-1] == fill + extra, (ref[2].sum(), fill, extra)
        _mixed(ref[0], f"total = 64 k + {extra}")
        _compare(dev.cloud_edge_validity(cloud, s, g, res, MAXD, threshold=thr, shapes=shapes), ref, f"total = 64 k + {extra}")
    # an edge of more than 128 samples between short ones; degenerate edges first, in the middle and last
    s, g = s0.copy(), g0.copy()
    g[20] = s[20] + (g[20] - s[20]) * (7.5 / np.linalg.norm(g[20] - s[20]))
    g[0] = s[0]                                                # start == goal
    s[19, 2] = np.nan                                          # a NaN start, dist = None: the norm is NaN
    s[39, 0] = np.nan
    ref = _ref(sm, pts, r, shapes, s, g, res, "connect", thr)
    assert ref[2][20] > 128 and ref[2].max() == ref[2][20] and np.median(ref[2]) < 10
    for e in (0, 19, 39):
        assert not ref[0][e] and ref[2][e] == 0 and np.isnan(ref[1][e]).all()
    assert ref[0][[1, 18, 21, 38]].any() and ref[0].sum() >= 10, "valid edges next to the degenerate ones"
    _compare(dev.cloud_edge_validity(cloud, s, g, res, MAXD, threshold=thr, shapes=shapes), ref, "long and degenerate edges")
    # a NaN start with a finite given dist: not degenerate, its count comes from dist, its samples are not finite
    s, g = s0.copy(), g0.copy()
    dist = np.linalg.norm(g - s, axis=1)
    s[7, 1] = np.nan
    dist[7] = 0.2
    for mode in MODES:
        ref = _ref(sm, pts, r, shapes, s, g, res, mode, thr, dist)
        assert not ref[0][7] and ref[2][7] == 5 and ref[0].sum() >= 10
        _compare(dev.cloud_edge_validity(cloud, s, g, res, MAXD, mode=mode, threshold=thr, dist=dist, shapes=shapes), ref, f"NaN start, given dist, {mode}")


# one edge of about 5 001 samples where the static bound (and so one pass of the grid) is 4 096: the kernel's stride serves the rest.
# From q[STRIDE_ROW] the last joint turns by 5 rad -- a free edge --; with joint STRIDE_JOINT moved by STRIDE_PUSH as well the arm
# reaches the scan only in the samples past the first pass
STRIDE_ROW, STRIDE_JOINT, STRIDE_PUSH = 1, 1, 0.7


def _stride_edge(q, push):
    s = q[STRIDE_ROW].copy()
    g = s.copy()
    g[-1] += 5.0
    g[STRIDE_JOINT] += push
    return s[None], g[None]


def test_cloud_edges_beyond_one_pass_of_the_grid(fresh_world, torch_cuda):
    from numbotics_amd.physics import PointCloud
    arm, keep, q = _robot("c1", True, None)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    shapes = list(range(1, sm.n_rshapes))
    N, r = CLOUDS[1]
    pts = _pts(N)
    cloud = PointCloud(pts, r)
    res = 1e-3
    for what, push in (("free", 0.0), ("colliding near its far end", STRIDE_PUSH)):
        s, g = _stride_edge(q, push)
        ref = _ref(sm, pts, r, shapes, s, g, res, "connect", 0.0)
        assert 4900 <= ref[2][0] <= 5100
        rows = edge_samples(s[0], g[0], res, MAXD, mode="connect")
        assert rows.shape[0] == ref[2][0]
        hits = cloud_mask(sm, pts, r, rows, 0.0, shapes)
        if push == 0.0:
            assert ref[0][0] and not hits.any()
        else:
            assert not ref[0][0] and hits.any() and not hits[:4096].any(), f"first hit at sample {np.flatnonzero(hits)[:1]}"
        _compare(dev.cloud_edge_validity(cloud, s, g, res, MAXD, shapes=shapes), ref, f"5 001 samples, {what}")


# ---- 3. accumulate ---------------------------------------------------------------------------------------------------------------
def test_cloud_edges_accumulate(fresh_world, torch_cuda):
    """edge_validity of c2 (its cube), then the cloud's verdicts ANDed into the same ``valid`` = the oracle on the combined model."""
    torch = torch_cuda
    from numbotics_amd import _lib
    from numbotics_amd.physics import PointCloud
    arm, keep, q = _robot("c2", True, None)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    shapes = list(range(1, sm.n_rshapes))
    N, r = CLOUDS[0]
    pts = _pts(N)
    cloud = PointCloud(pts, r)
    p = SETS["a"]
    s, g = edges(q, 200, 7, p["length"])
    st, gt = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
    for mode in MODES:
        own = Oracle(sm).edge_validity(s, g, p["resolution"], MAXD, mode=mode, threshold=p["thr"], nthreads=NT)
        only = _ref(sm, pts, r, shapes, s, g, p["resolution"], mode, p["thr"])
        both = _ref(sm, pts, r, shapes, s, g, p["resolution"], mode, p["thr"], keep_scene=True)
        assert np.array_equal(both[0], own[0] & only[0])
        assert (~own[0] & only[0]).sum() >= 3 and (own[0] & ~only[0]).sum() >= 3, "each side must block edges of its own"
        _mixed(both[0], f"combined {mode}")
        valid, end, ns = dev.edge_validity(st, gt, p["resolution"], MAXD, mode=mode, threshold=p["thr"])
        assert np.array_equal(valid.cpu().numpy(), own[0])
        got = dev.cloud_edge_validity(cloud, st, gt, p["resolution"], MAXD, mode=mode, threshold=p["thr"], shapes=shapes, out=valid)
        assert got[0] is valid
        _compare((valid.cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy()), both, f"accumulated {mode}")
        assert_bitwise(end.cpu().numpy(), got[1].cpu().numpy(), "the end states of the two calls")
        # uint8 as well; all zeros stay all zeros; all ones = the cloud alone
        for fill, want in ((0, np.zeros(200, dtype=bool)), (1, only[0]), (255, only[0])):
            out = torch.full((200,), fill, dtype=torch.uint8, device="cuda")
            dev.cloud_edge_validity(cloud, st, gt, p["resolution"], MAXD, mode=mode, threshold=p["thr"], shapes=shapes, out=out)
            assert np.array_equal(out.cpu().numpy(), want.astype(np.uint8)), f"out filled with {fill}"
        # an overwriting call ignores what valid held
        bits = dev._shape_bits(shapes)
        ws = torch.empty((dev.cloud_edge_workspace_bytes(200),), dtype=torch.uint8, device="cuda")
        for fill in (0, 7):
            out = torch.full((200,), fill, dtype=torch.uint8, device="cuda")
            rc = _lib.load().nbk_edge_cloud_validity_batch(dev._h, cloud._h, st.data_ptr(), gt.data_ptr(), None, 200, p["resolution"], MAXD,
                                                           MODES.index(mode), p["thr"], bits.ctypes.data, 0, out.data_ptr(), None, None,
                                                           ws.data_ptr(), ws.numel(), None)
            assert rc == 0
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), only[0].astype(np.uint8)), f"overwriting a valid filled with {fill}"
    for bad in (own[0], valid[:5], valid.float(), valid.cpu()):             # not a tensor; wrong shape, dtype, device
        with pytest.raises(ValueError, match="out must be"):
            dev.cloud_edge_validity(cloud, st, gt, p["resolution"], MAXD, shapes=shapes, out=bad)


# ---- 4. shape selection and the empty cases ----------------------------------------------------------------------------------------
def test_cloud_edges_selection_and_empty_cases(fresh_world, torch_cuda):
    from numbotics_amd.physics import PointCloud
    arm, keep, q = _robot("c1", True, None)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    S = sm.n_rshapes
    shapes = list(range(1, S))
    N, r = CLOUDS[1]
    pts = _pts(N)
    cloud = PointCloud(pts, r)
    p = SETS["b"]
    s, g = edges(q, 200, 7, p["length"])
    g[5] = s[5]                                                 # one degenerate edge
    kw = dict(mode="steer", threshold=p["thr"])
    ref = _ref(sm, pts, r, shapes, s, g, p["resolution"], "steer", p["thr"])
    _mixed(ref[0], "every shape but the base")
    last = _ref(sm, pts, r, [S - 1], s, g, p["resolution"], "steer", p["thr"])
    assert not last[0].all() and last[0].sum() > ref[0].sum(), "the selection matters"
    _compare(dev.cloud_edge_validity(cloud, s, g, p["resolution"], MAXD, shapes=[S - 1], **kw), last, "the last shape alone")
    # nothing to hit: every non-degenerate edge is valid
    free = (ref[2] > 0, ref[1], ref[2])
    assert not free[0][5] and free[0].sum() == 199
    _compare(dev.cloud_edge_validity(cloud, s, g, p["resolution"], MAXD, shapes=[], **kw), free, "empty selection")
    empty = PointCloud(np.zeros((0, 3)), r, bounds=([-1, -1, 0], [1, 1, 1]), capacity=8)
    _compare(dev.cloud_edge_validity(empty, s, g, p["resolution"], MAXD, shapes=shapes, **kw), free, "empty cloud")
    # a NaN point: every edge is invalid until a clean update
    bad = pts.copy()
    bad[123, 1] = np.nan
    cloud.update(bad)
    assert cloud.status() == 2
    _compare(dev.cloud_edge_validity(cloud, s, g, p["resolution"], MAXD, shapes=shapes, **kw), (np.zeros(200, dtype=bool), ref[1], ref[2]), "status set")
    cloud.update(pts)
    assert cloud.status() == 0
    _compare(dev.cloud_edge_validity(cloud, s, g, p["resolution"], MAXD, shapes=shapes, **kw), ref, "after a clean update")


# ---- 5. stream order and capture ---------------------------------------------------------------------------------------------------
def test_cloud_update_and_edges_in_one_graph(fresh_world, torch_cuda):
    """update + cloud_edge_validity captured on one side stream, every tensor static (the workspace among them); replays see the
    points tensor's current scan."""
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    arm, keep, q = _robot("c1", True, None)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    shapes = list(range(1, sm.n_rshapes))
    p = SETS["a"]
    s, g = edges(q, 200, 7, p["length"])
    sets = [_pts(300, seed=k) for k in (300, 41, 42, 43)]
    st, gt = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
    Pt = torch.from_numpy(sets[0].copy()).cuda()
    ws = torch.empty((dev.cloud_edge_workspace_bytes(200),), dtype=torch.uint8, device="cuda")
    cloud = PointCloud(Pt, 0.01, bounds=([-0.6, -0.6, 0.0], [0.6, 0.6, 1.0]))
    args = (cloud, st, gt, p["resolution"], MAXD)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dev.cloud_edge_validity(*args, threshold=p["thr"], shapes=shapes, workspace=ws)       # warm-up outside the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            cloud.update(Pt)
            valid, end, ns = dev.cloud_edge_validity(*args, threshold=p["thr"], shapes=shapes, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    refs = []
    for k in (1, 2, 3):
        Pt.copy_(torch.from_numpy(sets[k].copy()).cuda())
        graph.replay()
        torch.cuda.synchronize()
        ref = _ref(sm, sets[k], 0.01, shapes, s, g, p["resolution"], "connect", p["thr"])
        _mixed(ref[0], f"replay {k}")
        _compare((valid.cpu().numpy(), end.cpu().numpy(), ns.cpu().numpy()), ref, f"replay {k}")
        refs.append(ref[0].tobytes())
    assert len(set(refs)) == 3, "the three scans must differ in their verdicts"
    _compare(dev.cloud_edge_validity(cloud, s, g, p["resolution"], MAXD, threshold=p["thr"], shapes=shapes), ref, "a direct call sees the last scan")


# ---- 6. the C boundary on the device -----------------------------------------------------------------------------------------------
def test_cloud_edges_c_boundary(fresh_world, torch_cuda):
    torch = torch_cuda
    from numbotics_amd import _lib
    from numbotics_amd.physics import PointCloud
    lib = _lib.load()
    arm, keep, q = _robot("c1", True, None)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    shapes = list(range(1, sm.n_rshapes))
    N, r = CLOUDS[1]
    cloud = PointCloud(_pts(N), r)
    p = SETS["a"]
    E = 65
    s, g = edges(q, E, 7, p["length"])
    ref = _ref(sm, _pts(N), r, shapes, s, g, p["resolution"], "connect", p["thr"])
    st, gt = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
    need = lib.nbk_edge_cloud_workspace_bytes(E)
    ws = torch.zeros((need + 64,), dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 64 == 0
    valid = torch.full((E,), 9, dtype=torch.uint8, device="cuda")
    bits = dev._shape_bits(shapes)
    INVALID = -1

    def call(E_=E, wptr=ws.data_ptr(), wbytes=need, end=None, ns=None):
        return lib.nbk_edge_cloud_validity_batch(dev._h, cloud._h, st.data_ptr(), gt.data_ptr(), None, E_, p["resolution"], MAXD, 0, p["thr"],
                                                 bits.ctypes.data, 0, valid.data_ptr(), end, ns, wptr, wbytes, None)
    assert call(wbytes=need - 1) == INVALID
    assert call(wptr=ws.data_ptr() + 8, wbytes=need + 56) == INVALID
    torch.cuda.synchronize()
    assert (valid.cpu().numpy() == 9).all(), "a refused call writes nothing"
    assert call(E_=0) == 0 and call(E_=0, wptr=None, wbytes=0) == 0
    assert call() == 0                                          # null end and n_samples
    torch.cuda.synchronize()
    assert np.array_equal(valid.cpu().numpy(), ref[0].astype(np.uint8))
    end = torch.empty((E, sm.kin.n_q), dtype=torch.float64, device="cuda")
    assert call(end=end.data_ptr()) == 0
    torch.cuda.synchronize()
    assert_bitwise(end.cpu().numpy(), ref[1], "end alone")
    assert call(wptr=ws.data_ptr() + 64, wbytes=need) == 0     # any 64-byte aligned address serves
    torch.cuda.synchronize()
    assert np.array_equal(valid.cpu().numpy(), ref[0].astype(np.uint8))


# ---- 7. the connector --------------------------------------------------------------------------------------------------------------
def test_connector_with_a_cloud(fresh_world, torch_cuda):
    from numbotics_amd.physics import PointCloud
    from numbotics_amd.planning.sampling_based.connectors import ConnectorParams, DiscreteConnector
    arm, keep, q = _robot("c2", True, None)
    sm = arm.scene_model()
    N, r = CLOUDS[0]
    pts = _pts(N)
    cloud = PointCloud(pts, r)
    base = sm.links[sm.rshape_link[0]]._name
    shapes = [k for k in range(sm.n_rshapes) if sm.links[sm.rshape_link[k]]._name != base]
    assert 0 < len(shapes) < sm.n_rshapes
    p = SETS["a"]
    s, g = edges(q, 200, 7, p["length"])
    with_cloud = DiscreteConnector(ConnectorParams(arm=arm, cloud=cloud, cloud_ignore_links=(base,), resolution=0.05, max_distance=MAXD))
    without = DiscreteConnector(ConnectorParams(arm=arm, resolution=0.05, max_distance=MAXD))
    both = {m: _ref(sm, pts, r, shapes, s, g, 0.05, m, 0.0, keep_scene=True) for m in MODES}
    own = {m: Oracle(sm).edge_validity(s, g, 0.05, MAXD, mode=m, threshold=0.0, nthreads=NT) for m in MODES}
    for m in MODES:
        _mixed(both[m][0], f"connector {m}")
        assert (own[m][0] & ~both[m][0]).sum() >= 3, "the cloud must block edges the scene lets through"
    ok = with_cloud.connect_batch(s, g)
    assert ok.dtype == bool and np.array_equal(ok, both["connect"][0])
    ok, end = with_cloud.steer_batch(s, g)
    assert np.array_equal(ok, both["steer"][0])
    ok0, end0 = without.steer_batch(s, g)
    assert_bitwise(end, end0, "steer end states with and without a cloud")
    assert_bitwise(end, both["steer"][1], "steer end states")
    # the same connector without a cloud returns what it returned before
    assert np.array_equal(ok0, own["steer"][0]) and np.array_equal(without.connect_batch(s, g), own["connect"][0])
    # the scalar calls, from NumPy, on edges of both verdicts
    ref = both["connect"][0]
    pick = np.concatenate((np.flatnonzero(ref)[:4], np.flatnonzero(~ref)[:4]))
    for e in pick:
        out = with_cloud.connect(s[e], g[e])
        assert (out is not None) == bool(ref[e]), f"connect, edge {e}"
        if out is not None:
            assert_bitwise(out, g[e], "connect returns the goal")
        out = with_cloud.steer(s[e], g[e])
        assert (out is not None) == bool(both["steer"][0][e]), f"steer, edge {e}"
        if out is not None:
            assert_bitwise(out, both["steer"][1][e], "steer returns traj(T_f)")
    # is_valid: the scene's verdict ORed with the cloud's
    hit = Oracle(cloud_model(sm, pts, r, shapes, keep_scene=True)).validity(q[:16], 0.0)
    assert np.array_equal(hit, arm.in_collision(q[:16]) | arm.in_collision_with_cloud(q[:16], cloud, 0.0, (base,)))
    got = np.array([with_cloud.is_valid(q[b]) for b in range(16)])
    assert np.array_equal(got, ~hit)
    with pytest.raises(ValueError, match="do not see point clouds yet"):
        with_cloud.validate_trajectories(np.stack((s[:4], g[:4]), axis=1), degree=1)
