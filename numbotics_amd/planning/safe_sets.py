"""The data-parallel inner steps of the reference's IRIS solver on the device
(reference: numbotics/planning/safe_sets.py:124-134,164-201).

Only the collision-bound steps are provided; the convex programmes around them (hit-and-run sampling,
cvxpy/MOSEK ellipsoid, SLSQP) are out of scope.

* ``collision_mask(arm, points, tol)`` = ``[subject.in_collision(q, tol) for q in points]``, which upstream maps
  over a pool of cloned PyBullet worlds (safe_sets.py:186-191) -- here one launch.
* ``counter_example_bisection(arm, centre, points, num_bisections, tol)`` = ``counter_ex_search_bisection`` for
  every colliding sample at once (safe_sets.py:124-134): ``num_bisections`` launches on shrinking intervals
  instead of ``M * num_bisections`` single-configuration PyBullet queries.
* ``distance_and_gradient(arm, points, link, obj)`` = the constraint value and Jacobian that
  ``counter_ex_search_nlp`` hands to SLSQP (safe_sets.py:86-121: ``distance_to(x, link, obj)[0].distance`` and
  ``jacobian_proximity(x, link=link, obj=obj)``), for M points in one launch that computes the body pair's primitive pairs
  only (``Arm.pair_proximity_jacobians``).
* ``cloud_distance_and_gradient(arm, points, cloud, d_max, link)``: the same constraint value and gradient against a point cloud
  (``DeviceModel.cloud_records``), one launch.
"""
import numpy as np


def collision_mask(arm, points, collision_tolerance: float = 1e-6):
    """(M, dof) -> (M,) bool, True where the configuration's closest pair is nearer than the tolerance."""
    return arm.in_collision(points, collision_tolerance)


def counter_example_bisection(arm, centre, points, num_bisections: int = 15, collision_tolerance: float = 1e-6, graph: bool = False):
    """For each colliding point q: bisect [centre, q] keeping the colliding end, return the final upper ends.

    Same arithmetic per sample as upstream: ``midpoint = (lo + hi) / 2.0``; a colliding midpoint replaces
    ``hi``, a free one replaces ``lo``.

    ``points`` as a torch CUDA tensor keeps every round on the device -- midpoints, the validity launch and the interval
    update (``torch.where`` on the returned mask) with no copy through the host -- and returns a CUDA tensor, bit-equal to the
    NumPy form.  ``graph=True`` replays one captured round (midpoint, validity kernels, update: one graph launch instead of six)
    from a graph kept on the Arm per (scene, M, tolerance); the first such call pays for the capture."""
    if type(points).__module__.startswith("torch") and points.is_cuda:
        return _bisection_on_device(arm, centre, points, num_bisections, collision_tolerance, graph)
    points = np.asarray(points, dtype=np.float64)
    lo = np.tile(np.asarray(centre, dtype=np.float64)[None], (points.shape[0], 1))
    hi = points.copy()
    for _ in range(num_bisections):
        mid = (lo + hi) / 2.0
        hit = np.asarray(arm.in_collision(mid, collision_tolerance))
        hi[hit] = mid[hit]
        lo[~hit] = mid[~hit]
    return hi


class _Bisection:
    """Persistent buffers (lo, hi, mid, mask) of a bisection over M points; ``round()`` runs one round on the current stream."""

    def __init__(self, dev, M, nq, tol, device, ws_bytes=0):
        import torch
        from numbotics_amd import _lib
        self.dev, self.M, self.tol = dev, M, float(tol)
        self.lo = torch.empty((M, nq), dtype=torch.float64, device=device)
        self.hi = torch.empty_like(self.lo)
        self.mid = torch.empty_like(self.lo)
        self.mask = torch.empty((M,), dtype=torch.uint8, device=device)
        self.ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=device) if ws_bytes > 0 else None
        self._check = _lib.check

    def round(self):
        import torch
        torch.add(self.lo, self.hi, out=self.mid)
        self.mid.div_(2.0)                                # (lo + hi) / 2.0, as upstream
        d = self.dev
        ws = () if self.ws is None else (self.ws.data_ptr(), self.ws.numel())
        fn = d._lib.nbk_validity_batch_ws if ws else d._lib.nbk_validity_batch
        self._check(fn(d._h, self.mid.data_ptr(), self.M, self.tol, None, self.mask.data_ptr(), *ws, d._stream()), fn.__name__)
        hit = self.mask.bool().unsqueeze(1)
        torch.where(hit, self.mid, self.hi, out=self.hi)
        torch.where(hit, self.lo, self.mid, out=self.lo)


class _BisectionGraph(_Bisection):
    """One captured round on a private stream, for one (scene, M, tolerance), kept on the Arm: capturing costs more than a whole
    15-round search.  Its validity call uses a workspace of its own, never the library's per-stream scratch, which a later call on
    the same (pooled) stream may regrow; size 0 = the fused kernel, which keeps nothing between calls."""

    def __init__(self, dev, M, nq, tol, device):
        import torch
        super().__init__(dev, M, nq, tol, device, dev.validity_workspace_bytes(M))
        self.stream, self.graph = torch.cuda.Stream(), None

    def run(self, centre, pts, rounds):
        import torch
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            self.lo.copy_(centre.expand_as(self.lo))
            self.hi.copy_(pts)
            if self.graph is None:
                self.round()                              # one round outside the capture: lazy initialisation happens here
                rounds -= 1
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=self.stream):     # records one round, executes nothing
                    self.round()
                self.graph = g
            for _ in range(rounds):
                self.graph.replay()
            out = self.hi.clone()
        torch.cuda.current_stream().wait_stream(self.stream)
        return out


def _bisection_on_device(arm, centre, points, num_bisections, tol, graph):
    import torch
    pts = points.to(torch.float64).contiguous()
    M, nq = pts.shape
    c = torch.as_tensor(np.asarray(centre, dtype=np.float64), device=pts.device).reshape(1, nq)
    if M == 0 or num_bisections <= 0:
        return pts.clone()
    _, dev = arm._scene_device()
    if graph:
        cache = arm.__dict__.setdefault("_bisection_graphs", {})
        key = (id(dev), M, float(tol), pts.device.index)
        if key not in cache:
            if len(cache) >= 8:
                cache.clear()
            cache[key] = _BisectionGraph(dev, M, nq, tol, pts.device)
        return cache[key].run(c, pts, num_bisections)
    state = _Bisection(dev, M, nq, tol, pts.device)
    state.lo.copy_(c.expand(M, nq))
    state.hi.copy_(pts)
    for _ in range(num_bisections):
        state.round()
    return state.hi


def distance_and_gradient(arm, points, link, obj):
    """(M, dof) -> signed distance (M,) of the body pair (link, obj) and its gradient rows (M, dof).

    A body pair of compound links has several primitive pairs: the closest one is reported per point (for
    single-primitive links this is upstream's ``[0]``)."""
    sm, _ = arm._scene_device()
    if not arm._has(arm.collision_pairs(), link, obj):
        raise ValueError(f"Collision pair ({link.name}, {obj.name}) not valid")
    sel = arm._pair_selection(sm, obj, link)
    points = np.asarray(points, dtype=np.float64).reshape(-1, arm.dof)
    _, dev = arm._scene_device()
    dist, _, rows = arm._subset_records(dev, points, np.asarray(sel, dtype=np.int64), witness=False)   # the body pair's columns only
    k = np.argmin(dist, axis=1)
    i = np.arange(points.shape[0])
    return dist[i, k], rows[i, k]


def cloud_distance_and_gradient(arm, points, cloud, d_max, link=None, ignore_links=()):
    """``distance_and_gradient`` against a point cloud: (M, dof) -> the signed distance (M,) between the arm and ``cloud`` (a
    ``PointCloud``) where it is below ``d_max`` and its gradient rows (M, dof); inf and a row of zeros where nothing is that near
    (the value and gradient of a hinge constraint), NaN for a non-finite point.  ``link`` (a Link or its name): that link's shapes
    only, the minimum over them; otherwise every shape but those of ``ignore_links``."""
    sm = arm.scene_model()
    if link is not None:
        name = getattr(link, "_name", link)
        arm._cloud_shapes(sm, [name])                                    # an unknown link: its error
        shapes = [s for s in range(sm.n_rshapes) if sm.links[sm.rshape_link[s]]._name == name]
    else:
        shapes = arm._cloud_shapes(sm, ignore_links)
    points = np.asarray(points, dtype=np.float64).reshape(-1, arm.dof)
    _, dev = arm._scene_device()
    dist, _, _, _, rows = dev.cloud_records(cloud, points, d_max, shapes=shapes, witness=False)
    return dist, rows


def attached_distance_and_gradient(arm, points, att, pose=None):
    """``distance_and_gradient`` with an object in the hand: (M, dof) -> the signed distance (M,) of the closest item of the
    attachment ``att`` (held shape against a link or an obstacle it is paired with; the first minimum) and its gradient rows
    (M, dof); NaN for a non-finite point, inf and a row of zeros for an attachment without items.  ``pose``: another grasp, as
    ``Arm.in_collision_with_attached``."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, arm.dof)
    dist, _, _, rows = arm.attached_proximity_jacobians(points, att, pose=pose)
    return dist, rows
