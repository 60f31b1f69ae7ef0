"""The key of a certified call on the device ("the key of a certified call"), on the batches of tests/ca_key_cases.py: an
edge that collides at t = 0 (key 0) beside a degenerate one (CA_DEGENERATE_KEY), a cloud whose status is set and rows that come in
with a NaN t_free (CA_KEEP_KEY), each batch tiled across the 256-thread blocks of the init and final kernels.  Every copy of a batch
equals the restatement bit for bit.  Needs a real MI355X."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.cpu_oracle import Oracle
from numbotics_amd.planning import unit_knots
from test_gpu_parity import torch_cuda      # noqa: F401  (fixture)
import ca_key_cases as K
from ca_ref import UNDECIDED, DEGENERATE
from continuous_ref import reference_continuous
from spline_continuous_ref import reference_spline_continuous
from cloud_continuous_ref import reference_cloud_continuous


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _assert_rows(got, want, what):
    """got = (valid, t_free, status[, end]) of the device, want the same arrays of as many rows: equal bit for bit."""
    for name, a, b in zip(("valid", "t_free", "status", "end"), got, want):
        a, b = _host(a), np.asarray(b)
        if a.dtype.kind == "f":
            a, b = _bits(a), _bits(b)
        else:
            a, b = a.astype(np.int64), b.astype(np.int64)
        assert a.shape == b.shape, f"{what}: {name} has shape {a.shape}, expected {b.shape}"
        assert np.array_equal(a, b), f"{what}: {name} differs on rows {np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0][:10]}"


def _tiled_ref(valid, t_free, status, end=None):
    out = (K.tiled(valid), K.tiled(t_free), K.tiled(status))
    return out if end is None else out + (K.tiled(end),)


@pytest.mark.parametrize("max_iter", K.MAX_ITERS)
@pytest.mark.parametrize("mode", ["connect", "steer"])
def test_edges(fresh_world, torch_cuda, mode, max_iter):
    arm, chain, obs = K.scene()
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    s, g = K.edges(chain)
    rv, rend, rtf, rst, _, _ = reference_continuous(sm, Oracle(sm), s, g, K.MAX_DISTANCE[mode], mode=mode, max_iter=max_iter)
    valid, end, t_free, status = dev.edge_continuous(K.tiled(s), K.tiled(g), K.MAX_DISTANCE[mode], mode=mode, max_iter=max_iter)
    assert status.shape == (264,)
    _assert_rows((valid, t_free, status, end), _tiled_ref(rv, rtf, rst, rend), f"{mode} max_iter={max_iter}")


@pytest.mark.parametrize("max_iter", K.MAX_ITERS)
def test_splines(fresh_world, torch_cuda, max_iter):
    arm, chain, obs = K.scene()
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    c = K.splines(chain)
    ref = reference_spline_continuous(sm, Oracle(sm), c, unit_knots(4, 3), 3, max_iter=max_iter)
    got = dev.spline_continuous(K.tiled(c), unit_knots(4, 3), 3, max_iter=max_iter)
    assert got[2].shape == (268,)
    _assert_rows(got, _tiled_ref(*ref[:3]), f"splines max_iter={max_iter}")
    if max_iter == K.MAX_ITERS[0]:
        got = dev.spline_continuous(K.tiled(c), K.unclamped_knots(), 3)
        _assert_rows(got, (np.zeros(268, dtype=bool), np.full(268, np.nan), np.full(268, DEGENERATE, dtype=np.int32)), "knots not clamped")


@pytest.mark.parametrize("max_iter", K.MAX_ITERS)
def test_cloud_accumulates_into_the_scene(fresh_world, torch_cuda, max_iter):
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    arm, chain, obs = K.scene()
    sm = arm.scene_model()
    orc = Oracle(sm)
    _, dev = arm._scene_device()
    s, g = K.edges(chain)
    pts, shapes = K.cloud(sm)
    maxd = K.MAX_DISTANCE["connect"]
    kw = dict(max_iter=max_iter, look_ahead=K.CLOUD_LOOK_AHEAD, shapes=shapes)
    both = reference_cloud_continuous(sm, pts, K.CLOUD_R, s, g, maxd, scene_orc=orc, **kw)
    want = _tiled_ref(both[0], both[2], both[3], both[1])
    cloud = PointCloud(pts, K.CLOUD_R, bounds=K.CLOUD_BOX)
    st_, gt_ = torch.from_numpy(K.tiled(s)).cuda(), torch.from_numpy(K.tiled(g)).cuda()

    def accumulated(edit=None):
        valid, end, t_free, status = dev.edge_continuous(st_, gt_, maxd, max_iter=max_iter)
        if edit is not None:
            edit(valid, t_free, status)
        valid, end, t_free, status = dev.cloud_edge_continuous(cloud, st_, gt_, maxd, out=(valid, t_free, status), **kw)
        return valid, t_free, status, end

    _assert_rows(accumulated(), want, "accumulated")

    # rows that come in as the world guard leaves them keep 0 / NaN / UNDECIDED; the others are reduced as usual
    def guard_rows(valid, t_free, status):
        valid[:K.N_KEPT], t_free[:K.N_KEPT], status[:K.N_KEPT] = False, float("nan"), UNDECIDED
    kept = [a.copy() for a in want]
    kept[0][:K.N_KEPT], kept[1][:K.N_KEPT], kept[2][:K.N_KEPT] = False, np.nan, UNDECIDED
    _assert_rows(accumulated(guard_rows), kept, "rows with a NaN t_free coming in")

    # a non-finite point: every non-degenerate edge 0 / NaN / UNDECIDED, every degenerate one DEGENERATE, accumulating or not
    bad = pts.copy()
    bad[5, 2] = np.inf
    cloud.update(bad)
    assert cloud.status() == 2
    live = K.tiled(both[3] != DEGENERATE)
    unknown = (np.zeros(264, dtype=bool), np.full(264, np.nan), np.where(live, UNDECIDED, DEGENERATE).astype(np.int32), want[3])
    _assert_rows(accumulated(), unknown, "status set, accumulating")
    valid, end, t_free, status = dev.cloud_edge_continuous(cloud, st_, gt_, maxd, **kw)
    _assert_rows((valid, t_free, status, end), unknown, "status set")
