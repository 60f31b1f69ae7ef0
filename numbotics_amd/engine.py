"""Device engine: owns an ``nbk_model`` handle and launches the HIP kernels on torch-managed buffers.

PyTorch is plumbing only (device memory, the current HIP stream); every number is produced by
libnbk.so.  NumPy inputs are staged to the GPU and results are returned as NumPy; torch CUDA tensors
stay on the device.  Without a GPU every compute call raises ``NbkError`` -- there is no CPU path.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import NbkError


def _torch():
    import torch
    return torch


def _require_gpu():
    torch = _torch()
    if not torch.cuda.is_available():
        raise NbkError("no GPU visible: the numbotics_amd device path has no CPU fallback")
    return torch


class _Staged:
    """A float64 (B, n) device tensor plus how to hand results back."""

    def __init__(self, x, n_cols, what="q"):
        torch = _require_gpu()
        self.numpy = not torch.is_tensor(x)
        if self.numpy:
            a = np.ascontiguousarray(np.asarray(x, dtype=np.float64)).reshape(-1, n_cols)
            self.t = torch.from_numpy(a).to("cuda", non_blocking=False)
        else:
            if not x.is_cuda:
                x = x.to("cuda")
            self.t = x.to(torch.float64).contiguous().reshape(-1, n_cols)
        self.B = int(self.t.shape[0])
        self.device = self.t.device

    def out(self, t):
        return t.cpu().numpy() if self.numpy else t


def _host_f64(a, n):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64)).reshape(-1)
    if a.size != n:
        raise ValueError(f"expected {n} values, got {a.size}")
    return a


def _host_ptr(a):
    """The address of an optional host array (None stays None)."""
    return None if a is None else a.ctypes.data


def _mode_int(mode):
    """``mode`` of the edge entries as the library takes it: 0 connect, 1 steer."""
    return 0 if mode == "connect" else 1


def model_desc(model):
    """The ``nbk_model_desc`` of a KinematicModel or SceneModel (robots/model.py) -> (desc, arrays it points into).  Keep the
    second value alive as long as the first is used.  Needs no GPU."""
    kin = getattr(model, "kin", model)
    scene = model if hasattr(model, "kin") else None
    keep = []

    def ptr(a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.ctypes.data
    d = _lib.ModelDesc()
    d.n_q, d.n_joints = kin.n_q, kin.n_joints
    d.joint_parent = ptr(kin.joint_parent, np.int32)
    d.joint_type = ptr(kin.joint_type, np.int32)
    d.joint_qidx = ptr(kin.joint_qidx, np.int32)
    d.joint_rot = ptr(kin.joint_rot, np.float64)
    d.joint_trans = ptr(kin.joint_trans, np.float64)
    d.joint_slide = ptr(kin.joint_slide, np.float64)
    d.joint_axis = ptr(kin.joint_axis, np.float64)
    d.base_pose = ptr(kin.base_pose, np.float64)
    if scene is not None:
        d.n_rshapes, d.n_wshapes, d.n_pairs = scene.n_rshapes, scene.n_wshapes, scene.n_pairs
        d.rshape_frame = ptr(scene.rshape_frame, np.int32)
        d.rshape_type = ptr(scene.rshape_type, np.int32)
        d.rshape_local = ptr(scene.rshape_local, np.float64)
        d.rshape_param = ptr(scene.rshape_param, np.float64)
        d.wshape_type = ptr(scene.wshape_type, np.int32)
        d.wshape_pose = ptr(scene.wshape_pose, np.float64)
        d.wshape_param = ptr(scene.wshape_param, np.float64)
        d.pair_a = ptr(scene.pair_a, np.int32)
        d.pair_b = ptr(scene.pair_b, np.int32)
        d.n_hulls = scene.n_hulls
        d.hull_vert_begin = ptr(scene.hull_vert_begin, np.int32)
        d.hull_verts = ptr(scene.hull_verts, np.float64)
        d.hull_face_begin = ptr(scene.hull_face_begin, np.int32)
        d.hull_planes = ptr(scene.hull_planes, np.float64)
    return d, keep


def edge_motion_bounds(model, starts, goals):
    """Motion bounds mu (E, P) of the linear edges starts -> goals for every allowed pair of a SceneModel, in its pair order:
    |d_p(t) - d_p(t')| <= mu[e, p] |t - t'| on q(t) = (1-t) s + t g.  The routine nbk_edge_continuous_batch advances with, run on
    the host (nbk_edge_motion_bounds_host); no GPU needed."""
    n_q = getattr(model, "kin", model).n_q
    s = np.ascontiguousarray(np.asarray(starts, dtype=np.float64)).reshape(-1, n_q)
    g = np.ascontiguousarray(np.asarray(goals, dtype=np.float64)).reshape(-1, n_q)
    if s.shape != g.shape:
        raise ValueError("starts and goals must have the same shape")
    d, keep = model_desc(model)
    P = int(d.n_pairs)
    mu = np.empty((s.shape[0], P), dtype=np.float64)
    _lib.check(_lib.load().nbk_edge_motion_bounds_host(C.byref(d), s.ctypes.data, g.ctypes.data, s.shape[0], mu.ctypes.data),
               "nbk_edge_motion_bounds_host")
    del keep
    return mu


def edge_shape_motion_bounds(model, starts, goals):
    """Motion bounds mu (E, S) of the linear edges starts -> goals for every robot shape of a SceneModel, in its shape order, against
    a world that stands still: no point of shape s moves further than mu[e, s] |t - t'| between q(t) and q(t').  The routine
    nbk_edge_cloud_continuous_batch advances with, run on the host (nbk_edge_shape_motion_bounds_host); no GPU needed."""
    n_q = getattr(model, "kin", model).n_q
    s = np.ascontiguousarray(np.asarray(starts, dtype=np.float64)).reshape(-1, n_q)
    g = np.ascontiguousarray(np.asarray(goals, dtype=np.float64)).reshape(-1, n_q)
    if s.shape != g.shape:
        raise ValueError("starts and goals must have the same shape")
    d, keep = model_desc(model)
    mu = np.empty((s.shape[0], int(d.n_rshapes)), dtype=np.float64)
    _lib.check(_lib.load().nbk_edge_shape_motion_bounds_host(C.byref(d), s.ctypes.data, g.ctypes.data, s.shape[0], mu.ctypes.data),
               "nbk_edge_shape_motion_bounds_host")
    del keep
    return mu


def spline_motion_bounds(model, ctrl, knots, degree):
    """Motion bounds mu (S, n - degree, P) of S clamped B-splines ctrl (S, n, n_q) sharing the knots, per knot span ell (index
    ell - degree) and allowed pair: |d_p(t) - d_p(t')| <= mu[s, ell - degree, p] |t - t'| for t, t' in [knots[ell], knots[ell+1]].
    The routine nbk_spline_continuous_batch advances with, run on the host (nbk_spline_motion_bounds_host); no GPU needed.
    Entries of empty spans are 0."""
    n_q = getattr(model, "kin", model).n_q
    c = np.ascontiguousarray(np.asarray(ctrl, dtype=np.float64))
    if c.ndim != 3 or c.shape[2] != n_q:
        raise ValueError(f"control points must have shape (S, n, {n_q}), got {c.shape}")
    S, n = c.shape[:2]
    k = int(degree)
    if not 1 <= k < n:
        raise ValueError("degree must be at least 1 and less than the number of control points")
    kn = _host_f64(knots, n + k + 1)
    d, keep = model_desc(model)
    mu = np.zeros((S, n - k, int(d.n_pairs)), dtype=np.float64)
    _lib.check(_lib.load().nbk_spline_motion_bounds_host(C.byref(d), c.ctypes.data, S, n, k, kn.ctypes.data, mu.ctypes.data),
               "nbk_spline_motion_bounds_host")
    del keep
    return mu


def spline_shape_motion_bounds(model, ctrl, knots, degree):
    """Motion bounds mu (S, n - degree, R) of S clamped B-splines ctrl (S, n, n_q) sharing the knots, per knot span ell (index
    ell - degree) and robot shape of a SceneModel, in its shape order, against a world that stands still: no point of shape x moves
    further than mu[s, ell - degree, x] |t - t'| between q(t) and q(t') for t, t' in [knots[ell], knots[ell+1]].  The routine
    nbk_spline_cloud_continuous_batch advances with, run on the host (nbk_spline_shape_motion_bounds_host); no GPU needed.
    Entries of empty spans are 0."""
    n_q = getattr(model, "kin", model).n_q
    c = np.ascontiguousarray(np.asarray(ctrl, dtype=np.float64))
    if c.ndim != 3 or c.shape[2] != n_q:
        raise ValueError(f"control points must have shape (S, n, {n_q}), got {c.shape}")
    S, n = c.shape[:2]
    k = int(degree)
    if not 1 <= k < n:
        raise ValueError("degree must be at least 1 and less than the number of control points")
    kn = _host_f64(knots, n + k + 1)
    d, keep = model_desc(model)
    mu = np.zeros((S, n - k, int(d.n_rshapes)), dtype=np.float64)
    _lib.check(_lib.load().nbk_spline_shape_motion_bounds_host(C.byref(d), c.ctypes.data, S, n, k, kn.ctypes.data, mu.ctypes.data),
               "nbk_spline_shape_motion_bounds_host")
    del keep
    return mu


def _world_poses_host(poses, n_wshapes):
    """(W, 12) float64 C-contiguous from (W, 12) / (W, 3, 4) / (W, 4, 4) host input."""
    a = np.asarray(poses, dtype=np.float64)
    if a.ndim == 3 and a.shape[1:] == (4, 4):
        a = a[:, :3, :]
    if a.shape not in ((n_wshapes, 12), (n_wshapes, 3, 4)):
        raise ValueError(f"world poses must have shape ({n_wshapes}, 12) or ({n_wshapes}, 3, 4), got {a.shape}")
    return np.ascontiguousarray(a).reshape(n_wshapes, 12)


def world_reach_bounds(model, poses=None):
    """Static reach bounds (P,) of a SceneModel's pairs, in its pair order, at the world poses ``poses`` ((W, 12) / (W, 3, 4),
    default: the scene's own): a lower bound over ALL configurations of the distance of the two cores (margins not included),
    -inf for robot-robot pairs and for shapes behind a prismatic joint.  The routine k_world_update and nbk_model_create cull
    with, run on the host (nbk_world_reach_bounds_host); no GPU needed."""
    W = model.n_wshapes
    ps = _world_poses_host(model.wshape_pose if poses is None else poses, W)
    d, keep = model_desc(model)
    out = np.full((int(d.n_pairs),), -np.inf, dtype=np.float64)
    _lib.check(_lib.load().nbk_world_reach_bounds_host(C.byref(d), ps.ctypes.data, out.ctypes.data), "nbk_world_reach_bounds_host")
    del keep
    return out


def broad_spec_source(model, movable=False, world_radius=None):
    """The source the per-robot broadphase is compiled from for a SceneModel (bytes), or None when the robot does not take it;
    ``movable`` / ``world_radius`` as for DeviceModel.  Runs on the host (nbk_broad_spec_source[_movable]); no GPU needed."""
    lib = _lib.load()
    d, keep = model_desc(model)
    if movable:
        if world_radius is None:
            from numbotics_amd.robots.model import default_world_radius
            world_radius = default_world_radius(model)
        fn = lib.nbk_broad_spec_source_movable
        fn.argtypes, fn.restype = [C.c_void_p, C.c_double, C.c_char_p, C.c_int64], C.c_int64
        call = lambda buf, cap: fn(C.byref(d), float(world_radius), buf, cap)
    else:
        call = lambda buf, cap: lib.nbk_broad_spec_source(C.byref(d), buf, cap)
    n = call(None, 0)
    if n < 0:
        _lib.check(int(n), "nbk_broad_spec_source")
    if n == 0:
        return None
    buf = C.create_string_buffer(int(n))
    call(buf, n)
    del keep
    return buf.value


# default ``look_ahead`` of DeviceModel.cloud_edge_continuous and ContinuousConnector(cloud=...): the fastest value measured whose UNDECIDED
# count is no higher than without a cut (tools/cloud_time.py --only certified).  Until that table has its figures
# the default is no cut at all, the one value that meets the rule unmeasured.
CLOUD_LOOK_AHEAD = float("inf")


class DeviceModel:
    """Device descriptor built from a KinematicModel or SceneModel (robots/model.py): immutable, or -- ``movable=True`` --
    immutable except for the poses of its world shapes, which ``set_world_poses`` rewrites on the device without rebuilding
    anything (nbk_model_create_movable).  ``world_radius``: how far from the origin a world shape's centre may ever be (poses
    beyond it are refused on the device: see ``world_status``); default ``robots.model.default_world_radius(scene)``."""

    def __init__(self, model, movable=False, world_radius=None):
        kin = getattr(model, "kin", model)
        scene = model if hasattr(model, "kin") else None
        if world_radius is not None and not movable:
            raise ValueError("world_radius is meaningful for movable=True only")
        if movable:
            if scene is None:
                raise ValueError("a movable descriptor needs a SceneModel")
            if world_radius is None:
                from numbotics_amd.robots.model import default_world_radius
                world_radius = default_world_radius(scene)
            world_radius = float(world_radius)
            if not (0.0 <= world_radius < np.inf):
                raise ValueError(f"world_radius must be finite and >= 0, got {world_radius}")
        _require_gpu()
        lib = _lib.load()
        self.kin, self.scene = kin, scene
        self.movable, self.world_radius = bool(movable), world_radius
        d, keep = model_desc(model)
        h = C.c_void_p()
        if movable:
            _lib.check(lib.nbk_model_create_movable(C.byref(d), world_radius, C.byref(h)), "nbk_model_create_movable")
        else:
            _lib.check(lib.nbk_model_create(C.byref(d), C.byref(h)), "nbk_model_create")
        del keep
        self._h = h
        self._lib = lib
        self.n_q = kin.n_q
        self.n_pairs = scene.n_pairs if scene is not None else 0

    # ---- moving world bodies --------------------------------------------------------------------
    def set_world_poses(self, poses, stream_ordered=False):
        """Move the world shapes of a movable descriptor: ``poses`` (W, 12) or (W, 3, 4) float64 world poses in the scene's world
        shape order.  A torch CUDA tensor goes to nbk_model_set_world_poses on the current stream: asynchronous, no allocation, no
        host synchronisation, capturable -- later calls on that stream see the new poses (other streams: order them with events).
        A NumPy array goes to nbk_model_set_world_poses_host (returns when the update is done; work already queued on the current
        stream is waited for first), or, with ``stream_ordered=True``, is copied to the device through a pinned
        staging buffer of the descriptor (non-blocking; before the buffer is reused the host waits for the PREVIOUS update only,
        never for the checks queued after it) and issued on the current stream like a tensor: no allocation and no stream
        synchronisation per move.  Poses that are not finite or lie beyond ``world_radius`` are refused on the device: see ``world_status``."""
        if not getattr(self, "movable", False):
            raise NbkError("set_world_poses needs a descriptor made with movable=True (NBK_ERR_UNSUPPORTED)")
        W = self.scene.n_wshapes
        torch = _torch()
        if torch.is_tensor(poses):
            t = poses
            if not t.is_cuda or t.dtype != torch.float64:
                raise ValueError("world poses on the device must be a float64 CUDA tensor")
            if tuple(t.shape) not in ((W, 12), (W, 3, 4)):
                raise ValueError(f"world poses must have shape ({W}, 12) or ({W}, 3, 4), got {tuple(t.shape)}")
            if not t.is_contiguous():
                raise ValueError("world poses on the device must be contiguous")
        else:
            a = _world_poses_host(poses, W)
            if not stream_ordered:
                torch.cuda.current_stream().synchronize()
                _lib.check(self._lib.nbk_model_set_world_poses_host(self._h, a.ctypes.data), "nbk_model_set_world_poses_host")
                return
            t = self._stage_world_poses(torch, a)
        _lib.check(self._lib.nbk_model_set_world_poses(self._h, t.data_ptr(), self._stream()), "nbk_model_set_world_poses")
        if t is self.__dict__.get("_pose_dev"):
            self._pose_done.record()

    def _stage_world_poses(self, torch, a):
        """(W, 12) host poses -> the descriptor's device pose buffer, by a non-blocking copy from its pinned staging buffer on the
        current stream.  `set_world_poses` records ``_pose_done`` behind the update that reads the device buffer."""
        st = self.__dict__.get("_pose_stage")
        if st is None:
            st = self._pose_stage = torch.empty(a.shape, dtype=torch.float64).pin_memory()
            self._pose_dev = torch.empty(a.shape, dtype=torch.float64, device="cuda")
            self._pose_done = torch.cuda.Event()
        else:
            self._pose_done.synchronize()          # the previous copy and update are through with both buffers
        st.copy_(torch.from_numpy(a))
        self._pose_dev.copy_(st, non_blocking=True)
        return self._pose_dev

    def world_status(self) -> int:
        """0: the last update's poses were all applied; 1: a centre lay beyond ``world_radius``; 2: a pose was not finite.  While
        it is not 0 every configuration is reported colliding, every edge / trajectory invalid and every distance NaN.
        Synchronises."""
        out = C.c_int32(0)
        _lib.check(self._lib.nbk_model_world_status(self._h, C.byref(out)), "nbk_model_world_status")
        return int(out.value)

    def broad_kernel_used(self) -> int:
        """Diagnostic: the broadphase of the last validity call (nbk_broad_kernel_used)."""
        return int(self._lib.nbk_broad_kernel_used(self._h))

    def __del__(self):
        h = getattr(self, "_h", None)
        for fs in getattr(self, "_framesets", {}).values():
            try:
                self._lib.nbk_frameset_destroy(fs)
            except Exception:
                pass
        if h:
            try:
                self._lib.nbk_model_destroy(h)
            except Exception:
                pass
            self._h = None

    @staticmethod
    def _stream():
        return C.c_void_p(_torch().cuda.current_stream().cuda_stream)

    # ---- kinematics ----------------------------------------------------------------------------
    def _frame_args(self, frame, extra_local):
        fr = self.kin.frames[frame]
        local = fr.local if extra_local is None else fr.local @ extra_local
        path = np.ascontiguousarray(fr.path, dtype=np.int32)
        return path, np.ascontiguousarray(local[:3, :4], dtype=np.float64).reshape(12)

    def fk(self, q, frame, extra_local=None, local_pose=None):
        torch = _require_gpu()
        qs = _Staged(q, self.n_q)
        path, local = self._frame_args(frame, extra_local)
        out = torch.empty((qs.B, 4, 4), dtype=torch.float64, device=qs.device)
        lp = None
        if local_pose is not None:
            lp = _Staged(local_pose, 16, "local_pose")
            if lp.B != qs.B:
                raise ValueError("local_pose must have one 4x4 per configuration")
        _lib.check(self._lib.nbk_fk_batch(self._h, qs.t.data_ptr(), qs.B, path.ctypes.data, len(path),
                                          local.ctypes.data, None if lp is None else lp.t.data_ptr(),
                                          out.data_ptr(), self._stream()), "nbk_fk_batch")
        return qs.out(out)

    def fk_frames(self, q, frames, extra_locals=None):
        """Poses of several frames per configuration in one sweep: (B, len(frames), 4, 4), bit-identical to ``fk`` per frame.
        ``extra_locals``: optional {frame: 4x4} right factors (e.g. COM offsets)."""
        torch = _require_gpu()
        qs = _Staged(q, self.n_q)
        frames = list(frames)
        ex = extra_locals or {}
        key = (tuple(frames), tuple(sorted((k, np.asarray(v, dtype=np.float64).tobytes()) for k, v in ex.items())))
        cache = self.__dict__.setdefault("_framesets", {})
        fs = cache.get(key)
        if fs is None:
            joints = np.empty((len(frames),), dtype=np.int32)
            locs = np.empty((len(frames), 12), dtype=np.float64)
            for i, f in enumerate(frames):
                fr = self.kin.frames[f]
                local = fr.local if f not in ex else fr.local @ np.asarray(ex[f], dtype=np.float64)
                joints[i] = fr.joint
                locs[i] = np.ascontiguousarray(local[:3, :4]).reshape(12)
            h = C.c_void_p()
            _lib.check(self._lib.nbk_frameset_create(self._h, len(frames), joints.ctypes.data, locs.ctypes.data, C.byref(h)),
                       "nbk_frameset_create")
            fs = cache[key] = h
        out = torch.empty((qs.B, len(frames), 4, 4), dtype=torch.float64, device=qs.device)
        _lib.check(self._lib.nbk_fk_frames_batch(self._h, fs, qs.t.data_ptr(), qs.B, out.data_ptr(), self._stream()),
                   "nbk_fk_frames_batch")
        return qs.out(out)

    def jacobian(self, q, frame, extra_local=None, local_pose=None, global_pose=None):
        torch = _require_gpu()
        qs = _Staged(q, self.n_q)
        path, local = self._frame_args(frame, extra_local)
        out = torch.empty((qs.B, 6, self.n_q), dtype=torch.float64, device=qs.device)
        mode, pose = 0, None
        if local_pose is not None:
            mode, pose = 1, _Staged(local_pose, 16)
        elif global_pose is not None:
            mode, pose = 2, _Staged(global_pose, 16)
        if pose is not None and pose.B != qs.B:
            raise ValueError("pose must have one 4x4 per configuration")
        _lib.check(self._lib.nbk_jacobian_batch(self._h, qs.t.data_ptr(), qs.B, path.ctypes.data, len(path),
                                                local.ctypes.data, mode, None if pose is None else pose.t.data_ptr(),
                                                out.data_ptr(), self._stream()), "nbk_jacobian_batch")
        return qs.out(out)

    def ik(self, pose, q0, frame, extra_local=None, limits=None, tol=1e-6, max_iter=100, max_failures=15):
        """B damped-least-squares IK problems of one frame -> (success (B,) bool, q (B,n_q), |diff| (B,), steps (B,))."""
        torch = _require_gpu()
        qs = _Staged(q0, self.n_q)
        ps = _Staged(pose, 16, "pose")
        if ps.B != qs.B:
            raise ValueError("pose and q0 must have the same number of rows")
        path, local = self._frame_args(frame, extra_local)
        lim = None if limits is None else _host_f64(limits, 2 * self.n_q)
        q = torch.empty((qs.B, self.n_q), dtype=torch.float64, device=qs.device)
        ok = torch.empty((qs.B,), dtype=torch.uint8, device=qs.device)
        nrm = torch.empty((qs.B,), dtype=torch.float64, device=qs.device)
        it = torch.empty((qs.B,), dtype=torch.int32, device=qs.device)
        _lib.check(self._lib.nbk_ik_batch(self._h, ps.t.data_ptr(), qs.t.data_ptr(), qs.B, path.ctypes.data, len(path),
                                          local.ctypes.data, None if lim is None else lim.ctypes.data, float(tol),
                                          int(max_iter), int(max_failures), q.data_ptr(), ok.data_ptr(), nrm.data_ptr(),
                                          it.data_ptr(), self._stream()), "nbk_ik_batch")
        return qs.out(ok.bool()), qs.out(q), qs.out(nrm), qs.out(it)

    # ---- collision -----------------------------------------------------------------------------
    def validity_workspace_bytes(self, B: int) -> int:
        return int(self._lib.nbk_validity_workspace_bytes(self._h, int(B)))

    def validity(self, q, threshold=0.0, packed=False, workspace=None):
        """In-collision flags.  packed=False: (B,) bool; packed=True: (ceil(B/64),) int64 words
        (bit b%64 of word b//64), the form the multi-GPU all-gather moves.
        `workspace`: optional torch uint8 CUDA tensor of at least validity_workspace_bytes(B) bytes
        (caller-owned scratch: concurrent streams / graph capture); default = the descriptor's own."""
        torch = _require_gpu()
        qs = _Staged(q, self.n_q)
        words = mask = None
        if packed:
            words = torch.empty(((qs.B + 63) // 64,), dtype=torch.int64, device=qs.device)   # every word is written
        else:
            mask = torch.empty((qs.B,), dtype=torch.uint8, device=qs.device)
        wp = None if words is None else words.data_ptr()
        mp = None if mask is None else mask.data_ptr()
        if workspace is None:
            _lib.check(self._lib.nbk_validity_batch(self._h, qs.t.data_ptr(), qs.B, float(threshold), wp, mp,
                                                    self._stream()), "nbk_validity_batch")
        else:
            _lib.check(self._lib.nbk_validity_batch_ws(self._h, qs.t.data_ptr(), qs.B, float(threshold), wp, mp,
                                                       workspace.data_ptr(), workspace.numel() * workspace.element_size(),
                                                       self._stream()), "nbk_validity_batch_ws")
        return qs.out(words) if packed else qs.out(mask.bool())

    NARROW_BUILDS = ("k_narrow_bool", "k_narrow_pos", "k_narrow_pred", "k_narrow")

    def narrow_build(self, threshold=0.0) -> str:
        """Diagnostic: the narrowphase build ``validity`` launches for this scene at this threshold (bench.py reports it)."""
        return self.NARROW_BUILDS[int(self._lib.nbk_debug_narrow_variant(self._h, float(threshold)))]

    def last_tiling(self):
        """Diagnostic: (tiles, configurations per tile, pipelined) of this descriptor's last broadphase + narrowphase launch, a
        validity batch or the flat sample batch of an edge call (nbk_debug_last_tiling); ``pipelined`` is 1 when the odd tiles ran
        on the library's second stream.  (0, 0, 0) before the first such launch."""
        out = (C.c_int64 * 3)()
        _lib.check(self._lib.nbk_debug_last_tiling(self._h, out), "nbk_debug_last_tiling")
        return int(out[0]), int(out[1]), int(out[2])

    def validity_scalar(self, q, threshold=0.0) -> bool:
        """One configuration from host memory (the reference's scalar ``in_collision(q)``): pinned, device-mapped staging
        inside the library, one wait -- no torch tensors on the way."""
        a = np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
        if a.size != self.n_q:
            raise ValueError(f"expected {self.n_q} values, got {a.size}")
        out = C.c_int32(0)
        _lib.check(self._lib.nbk_validity_scalar_host(self._h, a.ctypes.data, float(threshold), C.byref(out)),
                   "nbk_validity_scalar_host")
        return bool(out.value)

    def edge_validity_scalar(self, start, goal, resolution, max_distance, mode="connect", threshold=0.0, dist=None):
        """One edge from host memory -> (valid, end state (n_q,), samples)."""
        s = np.ascontiguousarray(start, dtype=np.float64).reshape(-1)
        g = np.ascontiguousarray(goal, dtype=np.float64).reshape(-1)
        if s.size != self.n_q or g.size != self.n_q:
            raise ValueError(f"expected {self.n_q} values per end point")
        end = np.empty((self.n_q,), dtype=np.float64)
        ok, ns = C.c_int32(0), C.c_int32(0)
        _lib.check(self._lib.nbk_edge_validity_scalar_host(
            self._h, s.ctypes.data, g.ctypes.data, -1.0 if dist is None else float(dist), float(resolution), float(max_distance),
            _mode_int(mode), float(threshold), C.byref(ok), end.ctypes.data, C.byref(ns)),
            "nbk_edge_validity_scalar_host")
        return bool(ok.value), end, int(ns.value)

    def closest(self, q):
        torch = _require_gpu()
        qs = _Staged(q, self.n_q)
        d = torch.empty((qs.B,), dtype=torch.float64, device=qs.device)
        idx = torch.empty((qs.B,), dtype=torch.int32, device=qs.device)
        _lib.check(self._lib.nbk_closest_batch(self._h, qs.t.data_ptr(), qs.B, d.data_ptr(), idx.data_ptr(),
                                               self._stream()), "nbk_closest_batch")
        return qs.out(d), qs.out(idx)

    # ---- point-cloud obstacles (physics/pointcloud.py) -------------------------------------------------
    def _shape_bits(self, shapes):
        """``shapes``: None (every robot shape) or an iterable of robot shape indices (``SceneModel`` order) -> host words."""
        if shapes is None:
            return None
        if self.scene is None:
            raise ValueError("a shape selection needs a SceneModel")
        S = self.scene.n_rshapes
        words = np.zeros((max((S + 63) // 64, 1),), dtype=np.uint64)
        for s in shapes:
            s = int(s)
            if not 0 <= s < S:
                raise ValueError(f"robot shape {s} out of range (0..{S - 1})")
            words[s >> 6] |= np.uint64(1) << np.uint64(s & 63)
        return words

    @staticmethod
    def _mask_out(torch, out, want, packed=False):
        """``out`` of the cloud calls that OR / AND into a mask: a contiguous CUDA tensor of shape ``want``, uint8 / bool, or int64
        words when ``packed`` -> out."""
        if not (torch.is_tensor(out) and out.is_cuda and out.is_contiguous() and tuple(out.shape) == want
                and (out.dtype == torch.int64 if packed else out.dtype in (torch.uint8, torch.bool))):
            raise ValueError(f"out must be a contiguous CUDA tensor of shape {want} ({'int64' if packed else 'uint8 / bool'})")
        return out

    @staticmethod
    def _ptr(t):
        """``data_ptr()`` of an optional device tensor; None stays None (a null pointer)."""
        return None if t is None else t.data_ptr()

    def _mask_result(self, torch, out, B, packed, device):
        """The row mask of the verdict calls -- the caller's ``out`` (``_mask_out``) or a fresh one of ``validity``'s form for this
        ``packed`` -> (mask, pointer to it as packed words or None, pointer to it as bytes or None)."""
        want = ((B + 63) // 64,) if packed else (B,)
        if out is not None:
            res = self._mask_out(torch, out, want, packed)
        else:
            res = torch.empty(want, dtype=torch.int64 if packed else torch.uint8, device=device)
        return (res, res.data_ptr(), None) if packed else (res, None, res.data_ptr())

    def _edge_result(self, torch, out, s):
        """(valid, end, n_samples) of the sampled edge calls that AND into ``out``: valid is the caller's ``out`` (``_mask_out``) or
        fresh, end and n_samples are fresh."""
        valid = torch.empty((s.B,), dtype=torch.uint8, device=s.device) if out is None else self._mask_out(torch, out, (s.B,))
        return (valid, torch.empty((s.B, self.n_q), dtype=torch.float64, device=s.device),
                torch.empty((s.B,), dtype=torch.int32, device=s.device))

    @staticmethod
    def _workspace(torch, workspace, size, n, device):
        """The caller's ``workspace``, or by default ``size(n)`` bytes from torch's caching allocator -> (tensor, its bytes)."""
        ws = torch.empty((size(n),), dtype=torch.uint8, device=device) if workspace is None else workspace
        return ws, ws.numel() * ws.element_size()

    @staticmethod
    def _views(st, out, valid, *rest):
        """The ending of the calls that reduce into ``out``: the caller's tensors as they are, else ``st.out()`` views of the fresh
        ones with the verdict as bool."""
        if out is not None:
            return (valid,) + rest
        return (st.out(valid.bool()),) + tuple(st.out(x) for x in rest)

    def cloud_validity(self, cloud, q, threshold=0.0, packed=False, shapes=None, out=None):
        """In-collision flags of q against ``cloud`` ALONE (a ``PointCloud``): this descriptor's own pairs and world shapes play no
        part.  Bit for bit the verdict of a descriptor that holds the cloud's points as sphere world shapes paired with the selected
        robot shapes.  ``shapes``: robot shape indices to check (default: all).  ``out``: a CUDA mask of the form ``validity``
        returns for this ``packed`` (uint8 / bool (B,), or int64 words) to OR the verdicts INTO -- ``validity`` then
        ``cloud_validity(..., out=mask)`` gives full validity; it is returned.  Without ``out`` the result is as ``validity``'s."""
        torch = _require_gpu()
        qs = _Staged(q, self.n_q)
        bits = self._shape_bits(shapes)
        res, words, mask = self._mask_result(torch, out, qs.B, packed, qs.device)
        _lib.check(self._lib.nbk_cloud_validity_batch(
            self._h, cloud._h, qs.t.data_ptr(), qs.B, float(threshold), _host_ptr(bits),
            0 if out is None else 1, words, mask, self._stream()), "nbk_cloud_validity_batch")
        return out if out is not None else qs.out(res if packed else res.bool())

    def cloud_self_filter(self, points, q0, radius, padding=0.0, keep=None, shapes=None):
        """Take the robot's own image out of a frame's points (nbk_frame_cloud_self_filter): ``keep[i]`` goes to 0 iff point i, as a
        sphere of ``radius``, is closer than ``padding`` to a selected robot shape at the ONE configuration ``q0`` -- the
        predicate of ``cloud_validity`` with threshold = padding, so a cloud of the points kept reads free there, exactly.
        ``points``: (N, 3) float64, NumPy or a CUDA tensor; ``q0``: (n_q,), NumPy or a float64 CUDA tensor (read when the kernel
        runs).  ``keep``: an (N,) uint8 CUDA tensor to work on in place (zeros stay zeros) -- it is returned; without it every
        point starts kept and the result is a fresh uint8 tensor, or a NumPy bool array for NumPy ``points``.  ``shapes``: as
        ``cloud_validity``.  A non-finite ``q0`` removes nothing.  No allocation and capturable when everything is a CUDA tensor."""
        bits = self._shape_bits(shapes)                 # (argument errors come before the device is touched)
        torch = _require_gpu()
        ps = _Staged(points, 3, "points")
        qs = _Staged(q0, self.n_q)
        if qs.B != 1:
            raise ValueError(f"q0 must be one configuration of {self.n_q} values")
        if keep is None:
            k = torch.ones((ps.B,), dtype=torch.uint8, device=ps.device)
        else:
            k = keep
            if not (torch.is_tensor(k) and k.is_cuda and k.dtype == torch.uint8 and k.is_contiguous() and tuple(k.shape) == (ps.B,)):
                raise ValueError(f"keep must be a contiguous uint8 CUDA tensor of shape ({ps.B},)")
        _lib.check(self._lib.nbk_frame_cloud_self_filter(
            self._h, qs.t.data_ptr(), ps.t.data_ptr() if ps.B > 0 else None, ps.B, float(radius), float(padding), _host_ptr(bits),
            k.data_ptr() if ps.B > 0 else None, self._stream()), "nbk_frame_cloud_self_filter")
        if keep is not None:
            return keep
        return k.cpu().numpy().astype(bool) if ps.numpy else k

    def render_depth(self, q, camera_pose, intrinsics, height, width, near=0.01, far=1000.0, eps=1e-6, max_steps=256, shapes=None,
                     world=True, miss=0.0, out=None, labels=False, counts=None, frame="optical"):
        """Depth frames of the device scene, ray-cast on the current stream (nbk_render_depth_batch): the selected robot shapes at
        ``q`` and, with ``world``, the world shapes, sphere-traced on the exact shape distance -- a surface is where the collision
        predicates read distance 0.  ``q``: (n_q,) or (B, n_q), ``camera_pose``: one pose or (B, 4, 4) / (B, 3, 4), NumPy or
        float64 CUDA tensors (read when the kernel runs; ``frame`` as ``backproject``); one row serves every frame of the other's
        batch.  ``intrinsics``: (fx, fy, cx, cy) or a 3 x 3 matrix.  -> depth, a float32 CUDA tensor (B, height, width): the metric
        depth along the view axis (what ``backproject`` takes), ``miss`` where the ray meets nothing within [near, far] or stays
        undecided after ``max_steps`` steps.  ``labels=True``: (depth, label), label int32: the robot shape (``SceneModel`` order),
        ``n_rshapes + w`` for world shape w, -1 miss, -2 undecided.  ``counts``: an int64 CUDA tensor (3,) that receives (hit
        pixels, undecided pixels, distance evaluations).  ``out``: the depth tensor (or the (depth, label) pair) to write into.
        A hit stops within ``eps`` in front of the surface.  No allocation and capturable when everything is a CUDA tensor."""
        from numbotics_amd.physics.pointcloud import _intrinsics, _device_poses
        bits = self._shape_bits(shapes)                 # (argument errors come before the device is touched)
        fx, fy, cx, cy = _intrinsics(intrinsics)
        H, W = int(height), int(width)
        if H < 0 or W < 0:
            raise ValueError(f"height and width must not be negative, got {H} x {W}")
        if not (fx > 0.0 and fy > 0.0):
            raise ValueError("focal lengths must be positive")
        if not (float(near) >= 0.0 and float(far) > float(near)):
            raise ValueError(f"need 0 <= near < far, got near={near}, far={far}")
        if not float(eps) > 0.0:
            raise ValueError(f"eps must be positive, got {eps}")
        if not 1 <= int(max_steps) <= 4096:
            raise ValueError(f"max_steps must be in 1..4096, got {max_steps}")
        if frame not in ("optical", "numbotics"):
            raise ValueError(f"frame must be 'optical' or 'numbotics', got {frame!r}")
        torch = _require_gpu()
        qs = _Staged(q, self.n_q)
        T = _device_poses(torch, camera_pose, frame)
        Bt = int(T.shape[0]) if T.ndim == 3 else 1
        B = max(qs.B, Bt)
        if qs.B not in (1, B) or Bt not in (1, B):
            raise ValueError(f"q has {qs.B} rows and camera_pose {Bt}: each must be one or the batch")
        if B * H * W >= 1 << 31:
            raise ValueError("B * height * width must stay below 2^31")
        depth, label = (out if labels else (out, None)) if out is not None else (None, None)
        if depth is None:
            depth = torch.empty((B, H, W), dtype=torch.float32, device=qs.device)
        elif not (torch.is_tensor(depth) and depth.is_cuda and depth.dtype == torch.float32 and depth.is_contiguous() and depth.numel() == B * H * W):
            raise ValueError(f"out: depth must be a contiguous float32 CUDA tensor of {B} x {H} x {W} values")
        if labels:
            if label is None:
                label = torch.empty((B, H, W), dtype=torch.int32, device=qs.device)
            elif not (torch.is_tensor(label) and label.is_cuda and label.dtype == torch.int32 and label.is_contiguous() and label.numel() == B * H * W):
                raise ValueError(f"out: label must be a contiguous int32 CUDA tensor of {B} x {H} x {W} values")
        if counts is not None and not (torch.is_tensor(counts) and counts.is_cuda and counts.dtype == torch.int64 and counts.is_contiguous()
                                       and counts.numel() == 3):
            raise ValueError("counts must be a contiguous int64 CUDA tensor of 3 values")
        n = B * H * W
        _lib.check(self._lib.nbk_render_depth_batch(
            self._h, qs.t.data_ptr(), qs.B, T.data_ptr(), Bt, B, H, W, fx, fy, cx, cy, float(near), float(far), float(eps), int(max_steps),
            _host_ptr(bits), 1 if world else 0, float(miss), depth.data_ptr() if n > 0 else None,
            label.data_ptr() if (label is not None and n > 0) else None, None if counts is None else counts.data_ptr(), self._stream()),
            "nbk_render_depth_batch")
        return (depth, label) if labels else depth

    def cloud_clearance(self, cloud, q, d_max, shapes=None):
        """Per configuration the smallest signed distance to ``cloud`` over the selected robot shapes when it is below ``d_max``
        -> (distance (B,), robot shape (B,) int32, point index (B,) int32); +inf, -1, -1 where nothing is closer than ``d_max``;
        NaN, -1, -1 for a non-finite configuration or while the cloud's status is set.  Ties: smallest shape, then smallest point."""
        torch = _require_gpu()
        qs = _Staged(q, self.n_q)
        bits = self._shape_bits(shapes)
        d = torch.empty((qs.B,), dtype=torch.float64, device=qs.device)
        sh = torch.empty((qs.B,), dtype=torch.int32, device=qs.device)
        pt = torch.empty((qs.B,), dtype=torch.int32, device=qs.device)
        _lib.check(self._lib.nbk_cloud_clearance_batch(
            self._h, cloud._h, qs.t.data_ptr(), qs.B, float(d_max), _host_ptr(bits),
            d.data_ptr(), sh.data_ptr(), pt.data_ptr(), self._stream()), "nbk_cloud_clearance_batch")
        return qs.out(d), qs.out(sh), qs.out(pt)

    def cloud_records(self, cloud, q, d_max, shapes=None, per_shape=False, witness=True, jacobian=True):
        """``cloud_clearance``'s record with the contact and the way out of it (nbk_records_cloud_batch) -> (dist, shape, point,
        witness or None, rows or None).  ``per_shape=False``: one record per configuration, (B,), (B,), (B,), (B, 9), (B, n_q);
        dist, shape and point are ``cloud_clearance``'s bits.  ``per_shape=True``: one per (configuration, selected shape),
        (B, n_sel) ..., column j the j-th selected shape in ascending index, each entry ``cloud_clearance`` with that shape
        selected alone.  witness = point on the robot shape, point on the cloud point's sphere, unit normal from the point to the
        shape; rows = n . Jv_shape(point on the shape), the gradient of the distance.  Nothing nearer than ``d_max``: inf, -1, -1,
        NaN witness, a row of zeros; a non-finite configuration or a set cloud status: NaN, -1, -1, NaN, NaN."""
        bits = self._shape_bits(shapes)                 # (argument errors come before the device is touched)
        torch = _require_gpu()
        qs = _Staged(q, self.n_q)
        if per_shape:
            n_sel = len({int(s) for s in shapes}) if shapes is not None else (0 if self.scene is None else self.scene.n_rshapes)
            lead = (qs.B, n_sel)
        else:
            lead = (qs.B,)
        d = torch.empty(lead, dtype=torch.float64, device=qs.device)
        sh = torch.empty(lead, dtype=torch.int32, device=qs.device)
        pt = torch.empty(lead, dtype=torch.int32, device=qs.device)
        w = torch.empty(lead + (9,), dtype=torch.float64, device=qs.device) if witness else None
        j = torch.empty(lead + (self.n_q,), dtype=torch.float64, device=qs.device) if jacobian else None
        if d.numel() > 0:
            _lib.check(self._lib.nbk_records_cloud_batch(
                self._h, cloud._h, qs.t.data_ptr(), qs.B, float(d_max), _host_ptr(bits), 1 if per_shape else 0,
                d.data_ptr(), sh.data_ptr(), pt.data_ptr(), self._ptr(w),
                self._ptr(j), self._stream()), "nbk_records_cloud_batch")
        return qs.out(d), qs.out(sh), qs.out(pt), None if w is None else qs.out(w), None if j is None else qs.out(j)

    def pair_distances(self, q, witness=False):
        torch = _require_gpu()
        qs = _Staged(q, self.n_q)
        d = torch.empty((qs.B, self.n_pairs), dtype=torch.float64, device=qs.device)
        w = torch.empty((qs.B, self.n_pairs, 9), dtype=torch.float64, device=qs.device) if witness else None
        _lib.check(self._lib.nbk_pair_distances_batch(self._h, qs.t.data_ptr(), qs.B, d.data_ptr(),
                                                      self._ptr(w), self._stream()),
                   "nbk_pair_distances_batch")
        return (qs.out(d), qs.out(w)) if witness else qs.out(d)

    def proximity_jacobian(self, q):
        """(B,P) signed distances, (B,P,9) witnesses and (B,P,n_q) proximity-Jacobian rows of every allowed pair."""
        torch = _require_gpu()
        qs = _Staged(q, self.n_q)
        d = torch.empty((qs.B, self.n_pairs), dtype=torch.float64, device=qs.device)
        w = torch.empty((qs.B, self.n_pairs, 9), dtype=torch.float64, device=qs.device)
        j = torch.empty((qs.B, self.n_pairs, self.n_q), dtype=torch.float64, device=qs.device)
        _lib.check(self._lib.nbk_proximity_jacobian_batch(self._h, qs.t.data_ptr(), qs.B, d.data_ptr(), w.data_ptr(),
                                                          j.data_ptr(), self._stream()), "nbk_proximity_jacobian_batch")
        return qs.out(d), qs.out(w), qs.out(j)

    def _items(self, items, device):
        torch = _torch()
        if torch.is_tensor(items):
            t = items.to(device=device, dtype=torch.int32)
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(items, dtype=np.int32))).to(device)
        return t.contiguous().reshape(-1, 2)

    def _launch_records(self, qt, B, it, witness, jacobian):
        torch = _torch()
        N = int(it.shape[0])
        d = torch.empty((N,), dtype=torch.float64, device=qt.device)
        w = torch.empty((N, 9), dtype=torch.float64, device=qt.device) if witness else None
        j = torch.empty((N, self.n_q), dtype=torch.float64, device=qt.device) if jacobian else None
        _lib.check(self._lib.nbk_pair_records_items(self._h, qt.data_ptr(), B, it.data_ptr(), N, d.data_ptr(),
                                                    self._ptr(w), self._ptr(j),
                                                    self._stream()), "nbk_pair_records_items")
        return d, w, j

    def pair_records(self, q, items, witness=True, jacobian=True):
        """Records of chosen (configuration, pair) items: ``items`` (N, 2) int = (row of q, user pair index) ->
        dist (N,), witness (N, 9) or None, rows (N, n_q) or None -- the entries of ``proximity_jacobian(q)`` at [b, p], bit for
        bit; NaN for items outside [0, B) x [0, P)."""
        _require_gpu()
        qs = _Staged(q, self.n_q)
        it = self._items(items, qs.device)
        d, w, j = self._launch_records(qs.t, qs.B, it, witness, jacobian)
        return qs.out(d), None if w is None else qs.out(w), None if j is None else qs.out(j)

    def closest_records(self, q):
        """``closest`` followed by the records of each configuration's closest pair, with no host round trip in between:
        dist (B,), pair (B,) int32, witness (B, 9), rows (B, n_q)."""
        torch = _require_gpu()
        qs = _Staged(q, self.n_q)
        d = torch.empty((qs.B,), dtype=torch.float64, device=qs.device)
        idx = torch.empty((qs.B,), dtype=torch.int32, device=qs.device)
        _lib.check(self._lib.nbk_closest_batch(self._h, qs.t.data_ptr(), qs.B, d.data_ptr(), idx.data_ptr(),
                                               self._stream()), "nbk_closest_batch")
        it = torch.stack((torch.arange(qs.B, dtype=torch.int32, device=qs.device), idx), dim=1).contiguous()
        _, w, j = self._launch_records(qs.t, qs.B, it, True, True)
        return qs.out(d), qs.out(idx), qs.out(w), qs.out(j)

    def _stage_edges(self, starts, goals, dist):
        """The end points (and the optional lengths) of E edges on the device -> (starts, goals, dist or None), each ``_Staged``."""
        s = _Staged(starts, self.n_q)
        g = _Staged(goals, self.n_q)
        if s.B != g.B:
            raise ValueError("starts and goals must have the same number of rows")
        dd = None
        if dist is not None:
            dd = _Staged(dist, 1)
            if dd.B != s.B:
                raise ValueError("dist must have one value per edge")
        return s, g, dd

    def edge_validity(self, starts, goals, resolution, max_distance, mode="connect", threshold=0.0, dist=None):
        torch = _require_gpu()
        s, g, dd = self._stage_edges(starts, goals, dist)
        valid = torch.empty((s.B,), dtype=torch.uint8, device=s.device)
        end = torch.empty((s.B, self.n_q), dtype=torch.float64, device=s.device)
        ns = torch.empty((s.B,), dtype=torch.int32, device=s.device)
        _lib.check(self._lib.nbk_edge_validity_batch(
            self._h, s.t.data_ptr(), g.t.data_ptr(), None if dd is None else dd.t.data_ptr(), s.B,
            float(resolution), float(max_distance), _mode_int(mode), float(threshold),
            valid.data_ptr(), end.data_ptr(), ns.data_ptr(), self._stream()), "nbk_edge_validity_batch")
        return s.out(valid.bool()), s.out(end), s.out(ns)

    @staticmethod
    def cloud_edge_workspace_bytes(E: int) -> int:
        return int(_lib.load().nbk_edge_cloud_workspace_bytes(int(E)))

    def cloud_edge_validity(self, cloud, starts, goals, resolution, max_distance, mode="connect", threshold=0.0, dist=None, shapes=None,
                            out=None, workspace=None):
        """``edge_validity``'s edges against ``cloud`` ALONE (a ``PointCloud``): an edge is valid when it is not degenerate and
        ``cloud_validity`` clears every one of its samples (generated on the device, never stored) -> (valid (E,) bool, end (E, n_q),
        n_samples (E,) int32), ``end`` and ``n_samples`` bit for bit ``edge_validity``'s.  ``shapes``: as ``cloud_validity``.
        ``out``: a contiguous CUDA uint8 / bool (E,) tensor to AND the verdicts INTO -- entries that are already 0 stay 0 and cost
        nothing, so ``edge_validity`` then ``cloud_edge_validity(..., out=valid)`` is full edge validity; it is returned as the
        first element.  ``workspace``: optional torch uint8 CUDA tensor of at least ``cloud_edge_workspace_bytes(E)`` bytes; by
        default one is taken from torch's caching allocator (inside a graph capture: from the capture's pool)."""
        torch = _require_gpu()
        s, g, dd = self._stage_edges(starts, goals, dist)
        bits = self._shape_bits(shapes)
        valid, end, ns = self._edge_result(torch, out, s)
        ws, ws_bytes = self._workspace(torch, workspace, self.cloud_edge_workspace_bytes, s.B, s.device)
        _lib.check(self._lib.nbk_edge_cloud_validity_batch(
            self._h, cloud._h, s.t.data_ptr(), g.t.data_ptr(), None if dd is None else dd.t.data_ptr(), s.B, float(resolution),
            float(max_distance), _mode_int(mode), float(threshold), _host_ptr(bits),
            0 if out is None else 1, valid.data_ptr(), end.data_ptr(), ns.data_ptr(), ws.data_ptr(), ws_bytes,
            self._stream()), "nbk_edge_cloud_validity_batch")
        return self._views(s, out, valid)[0], s.out(end), s.out(ns)

    # ---- held objects (physics/attachment.py) ------------------------------------------------------------
    def _grasp(self, torch, pose, B, per_row):
        """``pose`` of the held calls -> (device tensor or None, rows): None (the stored grasp, 0 rows), (4, 4) (one) or, where
        ``per_row``, (B, 4, 4).  NumPy is staged; a float64 CUDA tensor is read in place when the kernel runs."""
        if pose is None:
            return None, 0
        if torch.is_tensor(pose):
            if not (pose.is_cuda and pose.dtype == torch.float64 and pose.is_contiguous()):
                raise ValueError("a pose on the device must be a contiguous float64 CUDA tensor")
            t = pose
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(pose, dtype=np.float64))).to("cuda")
        shape = tuple(t.shape)
        if shape == (4, 4):
            return t, 1
        if per_row and shape == (B, 4, 4):
            return t, B
        raise ValueError(f"pose must have shape (4, 4){f' or ({B}, 4, 4)' if per_row else ''}, got {shape}")

    def _held(self, held):
        if not isinstance(held, DeviceHeld) or held.dev is not self:
            raise ValueError("held must be a DeviceHeld made against this descriptor")
        return held._h

    def _held_scanless(self, held):
        """``_held`` for the held-versus-cloud calls: a held mesh sees scans only where its ``DeviceHeld`` was made with
        ``scans=True``; without that it is refused here, before the cloud or a device is touched (nbk.h answers
        NBK_ERR_UNSUPPORTED for it)."""
        h = self._held(held)
        if held.has_hull and not held.sees_scans:
            raise ValueError("held meshes do not see scans yet: the held-versus-cloud calls serve boxes, spheres, capsules and "
                             "cylinders only")
        return h

    def held_validity(self, held, q, threshold=0.0, packed=False, pose=None, out=None):
        """In-collision flags of q for the held object ``held`` (a ``DeviceHeld`` of this descriptor) ALONE: its shapes against the
        world shapes and robot shapes it was resolved against (nbk_held_validity_batch); this descriptor's own pairs play no part,
        and a copy of the object among the world shapes is still what ``validity`` sees.  ``pose``: the grasp -- the object's pose in
        the link frame -- (4, 4), or (B, 4, 4) with one grasp per row (screening grasp candidates); default: the stored one.  NumPy
        or a float64 CUDA tensor, which is read in place when the kernel runs, so a captured graph is re-grasped by rewriting it.  A
        row whose q or grasp is not finite collides.  ``packed`` / ``out``: as ``cloud_validity`` -- ``validity`` then
        ``held_validity(..., out=mask)`` is validity with the object in the hand."""
        torch = _require_gpu()
        h = self._held(held)
        qs = _Staged(q, self.n_q)
        g, rows = self._grasp(torch, pose, qs.B, True)
        res, words, mask = self._mask_result(torch, out, qs.B, packed, qs.device)
        _lib.check(self._lib.nbk_held_validity_batch(
            self._h, h, qs.t.data_ptr(), qs.B, self._ptr(g), rows, float(threshold),
            0 if out is None else 1, words, mask, self._stream()), "nbk_held_validity_batch")
        return out if out is not None else qs.out(res if packed else res.bool())

    @staticmethod
    def held_edge_workspace_bytes(E: int) -> int:
        return int(_lib.load().nbk_edge_held_workspace_bytes(int(E)))

    def held_edge_validity(self, held, starts, goals, resolution, max_distance, mode="connect", threshold=0.0, dist=None, pose=None,
                           out=None, workspace=None):
        """``edge_validity``'s edges for the held object ``held`` ALONE: an edge is valid when it is not degenerate and
        ``held_validity`` clears every one of its samples (nbk_edge_held_validity_batch) -> (valid (E,) bool, end (E, n_q),
        n_samples (E,) int32), ``end`` and ``n_samples`` bit for bit ``edge_validity``'s.  ``pose``: ONE grasp (4, 4) for the call,
        as ``held_validity``'s.  ``out`` / ``workspace``: as ``cloud_edge_validity`` (``held_edge_workspace_bytes(E)``)."""
        torch = _require_gpu()
        h = self._held(held)
        s, g, dd = self._stage_edges(starts, goals, dist)
        gr, _ = self._grasp(torch, pose, s.B, False)
        valid, end, ns = self._edge_result(torch, out, s)
        ws, ws_bytes = self._workspace(torch, workspace, self.held_edge_workspace_bytes, s.B, s.device)
        _lib.check(self._lib.nbk_edge_held_validity_batch(
            self._h, h, s.t.data_ptr(), g.t.data_ptr(), None if dd is None else dd.t.data_ptr(), s.B, float(resolution),
            float(max_distance), _mode_int(mode), float(threshold), self._ptr(gr),
            0 if out is None else 1, valid.data_ptr(), end.data_ptr(), ns.data_ptr(), ws.data_ptr(), ws_bytes,
            self._stream()), "nbk_edge_held_validity_batch")
        return self._views(s, out, valid)[0], s.out(end), s.out(ns)

    def held_distances(self, held, q, pose=None):
        """Signed distances of the items of ``held`` at q (nbk_held_distances_batch) -> (B, K): column k is item k of
        ``held.items()`` -- (held shape, robot shape) for the allowed robot shapes ascending, then (held shape, world shape) -- bit
        for bit ``pair_distances`` of a descriptor that holds the held shapes as robot shapes.  ``pose``: as ``held_validity``'s, one
        grasp or one per row.  NaN where the row or its grasp is not finite."""
        torch = _require_gpu()
        h = self._held(held)
        qs = _Staged(q, self.n_q)
        g, rows = self._grasp(torch, pose, qs.B, True)
        d = torch.empty((qs.B, held.n_items), dtype=torch.float64, device=qs.device)
        _lib.check(self._lib.nbk_held_distances_batch(
            self._h, h, qs.t.data_ptr(), qs.B, self._ptr(g), rows, d.data_ptr(), self._stream()),
            "nbk_held_distances_batch")
        return qs.out(d)

    @staticmethod
    def _check_items(items):
        """``items`` of ``held_records``: (N, 2) integers, NumPy or a tensor."""
        if _torch().is_tensor(items):
            shape, integer = tuple(items.shape), not (items.is_floating_point() or items.is_complex() or items.dtype == _torch().bool)
        else:
            a = np.asarray(items)
            shape, integer = a.shape, a.size == 0 or (np.issubdtype(a.dtype, np.integer) and a.dtype != np.bool_)
        if len(shape) != 2 or shape[1] != 2 or not integer:
            raise ValueError(f"items must be an (N, 2) integer array of (row of q, item index), got shape {shape}")

    def _launch_held_records(self, held, qt, B, g, rows, it, witness, jacobian):
        """The dense (``it`` None: (B, K) ...) or the listed (``it`` (N, 2) int32 on the device: (N,) ...) record kernel on device
        tensors -> (dist, witness or None, rows or None)."""
        torch = _torch()
        lead = (B, held.n_items) if it is None else (int(it.shape[0]),)
        d = torch.empty(lead, dtype=torch.float64, device=qt.device)
        w = torch.empty(lead + (9,), dtype=torch.float64, device=qt.device) if witness else None
        j = torch.empty(lead + (self.n_q,), dtype=torch.float64, device=qt.device) if jacobian else None
        gp, wp, jp = self._ptr(g), self._ptr(w), self._ptr(j)
        if d.numel() == 0:
            return d, w, j
        if it is None:
            _lib.check(self._lib.nbk_held_records_batch(self._h, held._h, qt.data_ptr(), B, gp, rows, d.data_ptr(), wp, jp, self._stream()),
                       "nbk_held_records_batch")
        else:
            _lib.check(self._lib.nbk_held_records_items(self._h, held._h, qt.data_ptr(), B, it.data_ptr(), int(it.shape[0]), gp, rows,
                                                        d.data_ptr(), wp, jp, self._stream()), "nbk_held_records_items")
        return d, w, j

    def held_records(self, held, q, pose=None, items=None, witness=True, jacobian=True):
        """``held_distances`` with the contact and the way out of it (nbk_held_records_batch / nbk_held_records_items) -> (dist,
        witness or None, rows or None).  ``items=None``: every item of every row, (B, K), (B, K, 9), (B, K, n_q), dist bit for bit
        ``held_distances``'.  ``items`` (N, 2) int = (row of q, item index of ``held.items()``), NumPy or a CUDA tensor: those
        entries only, (N,), (N, 9), (N, n_q) -- the dense ones at [b, k], NaN for an entry outside [0, B) x [0, K).  Bit for bit
        ``proximity_jacobian`` / ``pair_records`` of a descriptor that holds the held shapes as robot shapes: for a (held shape,
        robot shape) item the subject is the LINK's shape and the target the held shape, for a (held shape, world shape) item the
        subject is the held shape; witness = point on the subject, point on the target, unit normal from the target to the subject;
        rows = n . Jv_subject - n . Jv_target, the gradient of the distance.  ``pose``: as ``held_distances``'s (a listed item takes
        the grasp of its own row).  NaN in every field where the row or its grasp is not finite."""
        self._held(held)                                # (argument errors come before the device is touched)
        if items is not None:
            self._check_items(items)
        torch = _require_gpu()
        qs = _Staged(q, self.n_q)
        g, rows = self._grasp(torch, pose, qs.B, True)
        it = None if items is None else self._items(items, qs.device)
        d, w, j = self._launch_held_records(held, qs.t, qs.B, g, rows, it, witness, jacobian)
        return qs.out(d), None if w is None else qs.out(w), None if j is None else qs.out(j)

    def held_closest_records(self, held, q, pose=None):
        """``held_distances``, the closest item of every row (the first minimum) and that item's record, with no host round trip in
        between -> dist (B,), item (B,) int32, witness (B, 9), rows (B, n_q).  A row that is not finite gives NaN, -1, NaN, NaN; a
        held object without items inf, -1, NaN and rows of zeros."""
        self._held(held)
        torch = _require_gpu()
        qs = _Staged(q, self.n_q)
        g, rows = self._grasp(torch, pose, qs.B, True)
        B, K = qs.B, held.n_items
        if K == 0:
            return (qs.out(torch.full((B,), float("inf"), dtype=torch.float64, device=qs.device)),
                    qs.out(torch.full((B,), -1, dtype=torch.int32, device=qs.device)),
                    qs.out(torch.full((B, 9), float("nan"), dtype=torch.float64, device=qs.device)),
                    qs.out(torch.zeros((B, self.n_q), dtype=torch.float64, device=qs.device)))
        d = torch.empty((B, K), dtype=torch.float64, device=qs.device)
        _lib.check(self._lib.nbk_held_distances_batch(
            self._h, held._h, qs.t.data_ptr(), B, self._ptr(g), rows, d.data_ptr(), self._stream()),
            "nbk_held_distances_batch")
        bad = torch.isnan(d).any(dim=1)
        dmin = d.min(dim=1, keepdim=True).values
        k = torch.arange(K, dtype=torch.int32, device=qs.device).expand(B, K)
        first = torch.where(d == dmin, k, K).min(dim=1).values                      # the smallest index that attains the minimum
        item = torch.where(bad, -1, first).to(torch.int32)                          # (-1: out of range, every field NaN)
        it = torch.stack((torch.arange(B, dtype=torch.int32, device=qs.device), item), dim=1).contiguous()
        dist, w, j = self._launch_held_records(held, qs.t, B, g, rows, it, True, True)
        return qs.out(dist), qs.out(item), qs.out(w), qs.out(j)

    def held_edge_continuous(self, held, starts, goals, max_distance, mode="connect", threshold=0.0, max_iter=64, slack=1e-6, dist=None,
                             pose=None, out=None):
        """``edge_continuous``'s edges certified for the held object ``held`` ALONE (nbk_edge_held_continuous_batch): one (edge,
        held item) per lane advances by conservative advancement on the item's distance -> valid (E,) bool, end (E, n_q), t_free
        (E,), status (E,) int32 (``_lib.CA_*``).  ``pose``: ONE grasp (4, 4) for the call, as ``held_edge_validity``'s; a non-finite
        one gives 0 / NaN / UNDECIDED.  ``out``: the CUDA tensors (valid, t_free, status) that ``edge_continuous`` -- or
        ``cloud_edge_continuous(..., out=...)`` after it -- returned for the same edges, mode, max_distance and dist: the held items
        are reduced INTO them, as ``cloud_edge_continuous`` has it."""
        torch = _require_gpu()
        h = self._held(held)
        s, g, dd = self._stage_edges(starts, goals, dist)
        gr, _ = self._grasp(torch, pose, s.B, False)
        valid, t_free, status = self._result_triple(torch, out, s.B, s.device, "(valid, t_free, status)")
        end = torch.empty((s.B, self.n_q), dtype=torch.float64, device=s.device)
        _lib.check(self._lib.nbk_edge_held_continuous_batch(
            self._h, h, s.t.data_ptr(), g.t.data_ptr(), None if dd is None else dd.t.data_ptr(), s.B, float(max_distance),
            _mode_int(mode), float(threshold), int(max_iter), float(slack), self._ptr(gr),
            0 if out is None else 1, valid.data_ptr(), end.data_ptr(), t_free.data_ptr(), status.data_ptr(), self._stream()),
            "nbk_edge_held_continuous_batch")
        valid, t_free, status = self._views(s, out, valid, t_free, status)
        return valid, s.out(end), t_free, status

    @staticmethod
    def held_spline_workspace_bytes(S: int) -> int:
        return int(_lib.load().nbk_spline_held_workspace_bytes(int(S)))

    def held_spline_validity(self, held, ctrl, knots, degree, resolution, threshold=0.0, pose=None, out=None, workspace=None):
        """``spline_validity``'s trajectories for the held object ``held`` ALONE (nbk_spline_held_validity_batch): a trajectory is
        valid when it is not degenerate and ``held_validity`` clears every one of its samples -> (valid (S,) bool, t_hit (S,),
        n_samples (S,) int32).  Asynchronous on device tensors and capturable.  ``pose``: ONE grasp (4, 4) for the call; a
        non-finite one hits every trajectory at its first sample.  ``out``: the CUDA tensors (valid, t_hit, n_samples) that
        ``spline_validity`` -- or ``cloud_spline_validity(..., out=...)`` after it -- returned for the same trajectories and
        resolution: the held object's verdict is reduced INTO them, as ``cloud_spline_validity`` has it.  ``workspace``: optional
        torch uint8 CUDA tensor of at least ``held_spline_workspace_bytes(S)`` bytes."""
        torch = _require_gpu()
        h = self._held(held)
        c, kn, S, n = self._stage_splines(ctrl, knots, degree)
        gr, _ = self._grasp(torch, pose, S, False)
        valid, t_hit, ns = self._result_triple(torch, out, S, c.device, "(valid, t_hit, n_samples)")
        ws, ws_bytes = self._workspace(torch, workspace, self.held_spline_workspace_bytes, S, c.device)
        _lib.check(self._lib.nbk_spline_held_validity_batch(
            self._h, h, c.t.data_ptr(), S, n, int(degree), kn.data_ptr(), float(resolution), float(threshold),
            self._ptr(gr), 0 if out is None else 1, valid.data_ptr(), t_hit.data_ptr(), ns.data_ptr(),
            ws.data_ptr(), ws_bytes, self._stream()), "nbk_spline_held_validity_batch")
        return self._views(c, out, valid, t_hit, ns)

    def held_spline_continuous(self, held, ctrl, knots, degree, threshold=0.0, max_iter=64, slack=1e-6, pose=None, out=None):
        """``spline_continuous``'s trajectories certified for the held object ``held`` ALONE (nbk_spline_held_continuous_batch) ->
        valid (S,) bool, t_free (S,), status (S,) int32.  ``pose`` / ``out``: as ``held_edge_continuous``, ``out`` being what
        ``spline_continuous`` (or ``cloud_spline_continuous(..., out=...)`` after it) returned for the same trajectories."""
        torch = _require_gpu()
        h = self._held(held)
        c, kn, S, n = self._stage_splines(ctrl, knots, degree)
        gr, _ = self._grasp(torch, pose, S, False)
        valid, t_free, status = self._result_triple(torch, out, S, c.device, "(valid, t_free, status)")
        _lib.check(self._lib.nbk_spline_held_continuous_batch(
            self._h, h, c.t.data_ptr(), S, n, int(degree), kn.data_ptr(), float(threshold), int(max_iter), float(slack),
            self._ptr(gr), 0 if out is None else 1, valid.data_ptr(), t_free.data_ptr(), status.data_ptr(),
            self._stream()), "nbk_spline_held_continuous_batch")
        return self._views(c, out, valid, t_free, status)

    # ---- held objects against point clouds --------------------------------------------------------------
    def held_cloud_validity(self, held, cloud, q, threshold=0.0, packed=False, pose=None, out=None):
        """In-collision flags of q for the held object ``held`` against ``cloud`` (a ``PointCloud``) ALONE
        (nbk_held_cloud_validity_batch): no world shape and no link takes part, and the attachment's world list and robot set play
        none.  Bit for bit ``cloud_validity`` of a descriptor that holds the held shapes as robot shapes.  ``pose`` / ``packed`` /
        ``out``: as ``held_validity`` -- ``validity``, ``cloud_validity``, ``held_validity`` and this call on one mask are validity
        with the object in the hand among what the camera sees.  A row whose q or grasp is not finite collides, every row while
        the cloud's status is set; an empty cloud is free."""
        torch = _require_gpu()
        h = self._held_scanless(held)
        qs = _Staged(q, self.n_q)
        g, rows = self._grasp(torch, pose, qs.B, True)
        res, words, mask = self._mask_result(torch, out, qs.B, packed, qs.device)
        _lib.check(self._lib.nbk_held_cloud_validity_batch(
            self._h, h, cloud._h, qs.t.data_ptr(), qs.B, self._ptr(g), rows, float(threshold),
            0 if out is None else 1, words, mask, self._stream()), "nbk_held_cloud_validity_batch")
        return out if out is not None else qs.out(res if packed else res.bool())

    def held_cloud_clearance(self, held, cloud, q, d_max, pose=None):
        """Per configuration the smallest signed distance from the held object to ``cloud`` when it is below ``d_max``
        (nbk_held_cloud_clearance_batch) -> (distance (B,), held shape (B,) int32, point index (B,) int32); +inf, -1, -1 where
        nothing is closer than ``d_max``; NaN, -1, -1 for a non-finite configuration or grasp or while the cloud's status is set.
        Ties: smallest held shape, then smallest point.  ``pose``: as ``held_validity``'s, one grasp or one per row."""
        torch = _require_gpu()
        h = self._held_scanless(held)
        qs = _Staged(q, self.n_q)
        g, rows = self._grasp(torch, pose, qs.B, True)
        d = torch.empty((qs.B,), dtype=torch.float64, device=qs.device)
        sh = torch.empty((qs.B,), dtype=torch.int32, device=qs.device)
        pt = torch.empty((qs.B,), dtype=torch.int32, device=qs.device)
        _lib.check(self._lib.nbk_held_cloud_clearance_batch(
            self._h, h, cloud._h, qs.t.data_ptr(), qs.B, self._ptr(g), rows, float(d_max),
            d.data_ptr(), sh.data_ptr(), pt.data_ptr(), self._stream()), "nbk_held_cloud_clearance_batch")
        return qs.out(d), qs.out(sh), qs.out(pt)

    def held_cloud_records(self, held, cloud, q, d_max, pose=None, per_shape=False, witness=True, jacobian=True):
        """``held_cloud_clearance``'s record with the contact and the way out of it (nbk_held_cloud_records_batch) -> (dist, held
        shape, point, witness or None, rows or None), as ``cloud_records`` with the held shapes in the robot shapes' place.
        ``per_shape=False``: one record per configuration, (B,), (B,), (B,), (B, 9), (B, n_q); dist, shape and point are
        ``held_cloud_clearance``'s bits.  ``per_shape=True``: one per (configuration, held shape), (B, H) ..., column h the
        clearance of held shape h alone.  witness = point on the held shape, point on the cloud point's sphere, unit normal from the
        point to the shape; rows = n . Jv_held(point on the shape), the gradient of the distance.  Nothing nearer than ``d_max``:
        inf, -1, -1, NaN witness, a row of zeros; a non-finite configuration or grasp or a set cloud status: NaN, -1, -1, NaN, NaN.
        ``pose``: as ``held_validity``'s, one grasp or one per row."""
        h = self._held_scanless(held)
        torch = _require_gpu()
        qs = _Staged(q, self.n_q)
        g, rows = self._grasp(torch, pose, qs.B, True)
        lead = (qs.B, held.n_shapes) if per_shape else (qs.B,)
        d = torch.empty(lead, dtype=torch.float64, device=qs.device)
        sh = torch.empty(lead, dtype=torch.int32, device=qs.device)
        pt = torch.empty(lead, dtype=torch.int32, device=qs.device)
        w = torch.empty(lead + (9,), dtype=torch.float64, device=qs.device) if witness else None
        j = torch.empty(lead + (self.n_q,), dtype=torch.float64, device=qs.device) if jacobian else None
        if d.numel() > 0:
            _lib.check(self._lib.nbk_held_cloud_records_batch(
                self._h, h, cloud._h, qs.t.data_ptr(), qs.B, self._ptr(g), rows, float(d_max),
                1 if per_shape else 0, d.data_ptr(), sh.data_ptr(), pt.data_ptr(), self._ptr(w),
                self._ptr(j), self._stream()), "nbk_held_cloud_records_batch")
        return qs.out(d), qs.out(sh), qs.out(pt), None if w is None else qs.out(w), None if j is None else qs.out(j)

    @staticmethod
    def held_cloud_edge_workspace_bytes(E: int) -> int:
        return int(_lib.load().nbk_edge_held_cloud_workspace_bytes(int(E)))

    def held_cloud_edge_validity(self, held, cloud, starts, goals, resolution, max_distance, mode="connect", threshold=0.0, dist=None,
                                 pose=None, out=None, workspace=None):
        """``edge_validity``'s edges for the held object against ``cloud`` ALONE: an edge is valid when it is not degenerate and
        ``held_cloud_validity`` clears every one of its samples (nbk_edge_held_cloud_validity_batch) -> (valid (E,) bool, end
        (E, n_q), n_samples (E,) int32).  ``pose``: ONE grasp (4, 4) for the call.  ``out`` / ``workspace``: as
        ``cloud_edge_validity`` (``held_cloud_edge_workspace_bytes(E)``)."""
        torch = _require_gpu()
        h = self._held_scanless(held)
        s, g, dd = self._stage_edges(starts, goals, dist)
        gr, _ = self._grasp(torch, pose, s.B, False)
        valid, end, ns = self._edge_result(torch, out, s)
        ws, ws_bytes = self._workspace(torch, workspace, self.held_cloud_edge_workspace_bytes, s.B, s.device)
        _lib.check(self._lib.nbk_edge_held_cloud_validity_batch(
            self._h, h, cloud._h, s.t.data_ptr(), g.t.data_ptr(), None if dd is None else dd.t.data_ptr(), s.B, float(resolution),
            float(max_distance), _mode_int(mode), float(threshold), self._ptr(gr),
            0 if out is None else 1, valid.data_ptr(), end.data_ptr(), ns.data_ptr(), ws.data_ptr(), ws_bytes,
            self._stream()), "nbk_edge_held_cloud_validity_batch")
        return self._views(s, out, valid)[0], s.out(end), s.out(ns)

    @staticmethod
    def held_cloud_spline_workspace_bytes(S: int) -> int:
        return int(_lib.load().nbk_spline_held_cloud_workspace_bytes(int(S)))

    def held_cloud_spline_validity(self, held, cloud, ctrl, knots, degree, resolution, threshold=0.0, pose=None, out=None,
                                   workspace=None):
        """``spline_validity``'s trajectories for the held object against ``cloud`` ALONE (nbk_spline_held_cloud_validity_batch) ->
        (valid (S,) bool, t_hit (S,), n_samples (S,) int32).  ``pose``: ONE grasp (4, 4) for the call.  ``out`` / ``workspace``: as
        ``held_spline_validity`` (``held_cloud_spline_workspace_bytes(S)``)."""
        torch = _require_gpu()
        h = self._held_scanless(held)
        c, kn, S, n = self._stage_splines(ctrl, knots, degree)
        gr, _ = self._grasp(torch, pose, S, False)
        valid, t_hit, ns = self._result_triple(torch, out, S, c.device, "(valid, t_hit, n_samples)")
        ws, ws_bytes = self._workspace(torch, workspace, self.held_cloud_spline_workspace_bytes, S, c.device)
        _lib.check(self._lib.nbk_spline_held_cloud_validity_batch(
            self._h, h, cloud._h, c.t.data_ptr(), S, n, int(degree), kn.data_ptr(), float(resolution), float(threshold),
            self._ptr(gr), 0 if out is None else 1, valid.data_ptr(), t_hit.data_ptr(), ns.data_ptr(),
            ws.data_ptr(), ws_bytes, self._stream()), "nbk_spline_held_cloud_validity_batch")
        return self._views(c, out, valid, t_hit, ns)

    def held_cloud_edge_continuous(self, held, cloud, starts, goals, max_distance, mode="connect", threshold=0.0, max_iter=64,
                                   slack=1e-6, look_ahead=CLOUD_LOOK_AHEAD, dist=None, pose=None, out=None):
        """``edge_continuous``'s edges certified for the held object ``held`` against ``cloud`` ALONE
        (nbk_edge_held_cloud_continuous_batch): one (edge, held shape) item per lane advances by conservative advancement on the held
        shape's clearance from the cloud -> valid (E,) bool, end (E, n_q), t_free (E,), status (E,) int32 (``_lib.CA_*``).  No world
        shape and no link takes part.  Bit for bit ``cloud_edge_continuous`` of a descriptor that holds the held shapes as robot
        shapes, selected on those shapes.  ``look_ahead``: as ``cloud_edge_continuous``.  ``pose``: ONE grasp (4, 4) for the call, as
        ``held_edge_continuous``'s; a non-finite one, or a set cloud status, gives 0 / NaN / UNDECIDED; an empty cloud leaves every
        edge FREE at its stop point.  ``out``: the CUDA tensors (valid, t_free, status) of an earlier certified call on the same
        edges, mode, max_distance and dist (``edge_continuous``, then ``cloud_edge_continuous(..., out=...)`` and
        ``held_edge_continuous(..., out=...)``): these items are reduced INTO them."""
        torch = _require_gpu()
        h = self._held_scanless(held)
        s, g, dd = self._stage_edges(starts, goals, dist)
        gr, _ = self._grasp(torch, pose, s.B, False)
        valid, t_free, status = self._result_triple(torch, out, s.B, s.device, "(valid, t_free, status)")
        end = torch.empty((s.B, self.n_q), dtype=torch.float64, device=s.device)
        _lib.check(self._lib.nbk_edge_held_cloud_continuous_batch(
            self._h, h, cloud._h, s.t.data_ptr(), g.t.data_ptr(), None if dd is None else dd.t.data_ptr(), s.B, float(max_distance),
            _mode_int(mode), float(threshold), int(max_iter), float(slack), float(look_ahead),
            self._ptr(gr), 0 if out is None else 1, valid.data_ptr(), end.data_ptr(), t_free.data_ptr(),
            status.data_ptr(), self._stream()), "nbk_edge_held_cloud_continuous_batch")
        valid, t_free, status = self._views(s, out, valid, t_free, status)
        return valid, s.out(end), t_free, status

    def held_cloud_spline_continuous(self, held, cloud, ctrl, knots, degree, threshold=0.0, max_iter=64, slack=1e-6,
                                     look_ahead=CLOUD_LOOK_AHEAD, pose=None, out=None):
        """``spline_continuous``'s trajectories certified for the held object ``held`` against ``cloud`` ALONE
        (nbk_spline_held_cloud_continuous_batch) -> valid (S,) bool, t_free (S,), status (S,) int32.  ``look_ahead`` / ``pose`` /
        ``out``: as ``held_cloud_edge_continuous``, ``out`` being what an earlier certified spline call returned for the same
        trajectories."""
        torch = _require_gpu()
        h = self._held_scanless(held)
        c, kn, S, n = self._stage_splines(ctrl, knots, degree)
        gr, _ = self._grasp(torch, pose, S, False)
        valid, t_free, status = self._result_triple(torch, out, S, c.device, "(valid, t_free, status)")
        _lib.check(self._lib.nbk_spline_held_cloud_continuous_batch(
            self._h, h, cloud._h, c.t.data_ptr(), S, n, int(degree), kn.data_ptr(), float(threshold), int(max_iter), float(slack),
            float(look_ahead), self._ptr(gr), 0 if out is None else 1, valid.data_ptr(), t_free.data_ptr(),
            status.data_ptr(), self._stream()), "nbk_spline_held_cloud_continuous_batch")
        return self._views(c, out, valid, t_free, status)

    def edge_continuous(self, starts, goals, max_distance, mode="connect", threshold=0.0, max_iter=64, slack=1e-6, dist=None):
        """Certified continuous check of the linear edges starts -> goals (nbk_edge_continuous_batch) ->
        valid (E,) bool, end (E, n_q), t_free (E,), status (E,) int32 (``_lib.CA_*``)."""
        torch = _require_gpu()
        s, g, dd = self._stage_edges(starts, goals, dist)
        valid = torch.empty((s.B,), dtype=torch.uint8, device=s.device)
        end = torch.empty((s.B, self.n_q), dtype=torch.float64, device=s.device)
        t_free = torch.empty((s.B,), dtype=torch.float64, device=s.device)
        status = torch.empty((s.B,), dtype=torch.int32, device=s.device)
        _lib.check(self._lib.nbk_edge_continuous_batch(
            self._h, s.t.data_ptr(), g.t.data_ptr(), None if dd is None else dd.t.data_ptr(), s.B, float(max_distance),
            _mode_int(mode), float(threshold), int(max_iter), float(slack), valid.data_ptr(), end.data_ptr(),
            t_free.data_ptr(), status.data_ptr(), self._stream()), "nbk_edge_continuous_batch")
        return s.out(valid.bool()), s.out(end), s.out(t_free), s.out(status)

    def cloud_edge_continuous(self, cloud, starts, goals, max_distance, mode="connect", threshold=0.0, max_iter=64, slack=1e-6,
                              look_ahead=CLOUD_LOOK_AHEAD, dist=None, shapes=None, out=None):
        """``edge_continuous``'s edges certified against ``cloud`` ALONE (a ``PointCloud``; nbk_edge_cloud_continuous_batch): one
        (edge, robot shape) item per lane advances by conservative advancement on the shape's clearance from the cloud -> valid (E,)
        bool, end (E, n_q), t_free (E,), status (E,) int32 (``_lib.CA_*``).  ``shapes``: as ``cloud_validity``.  ``look_ahead`` (> 0,
        ``inf`` allowed): how far beyond threshold + slack one step searches the cloud; it changes the number of steps, never the
        soundness of FREE.  ``out``: the CUDA tensors (valid (E,) uint8 / bool, t_free (E,) float64, status (E,) int32) that
        ``edge_continuous`` returned for the same edges, mode, max_distance and dist: the cloud's items are reduced INTO them -- the
        result is that of one certified call over the scene's pairs and the cloud together; they are returned, with this call's end."""
        torch = _require_gpu()
        s, g, dd = self._stage_edges(starts, goals, dist)
        bits = self._shape_bits(shapes)
        valid, t_free, status = self._result_triple(torch, out, s.B, s.device, "(valid, t_free, status)")
        end = torch.empty((s.B, self.n_q), dtype=torch.float64, device=s.device)
        _lib.check(self._lib.nbk_edge_cloud_continuous_batch(
            self._h, cloud._h, s.t.data_ptr(), g.t.data_ptr(), None if dd is None else dd.t.data_ptr(), s.B, float(max_distance),
            _mode_int(mode), float(threshold), int(max_iter), float(slack), float(look_ahead),
            _host_ptr(bits), 0 if out is None else 1, valid.data_ptr(), end.data_ptr(), t_free.data_ptr(),
            status.data_ptr(), self._stream()), "nbk_edge_cloud_continuous_batch")
        valid, t_free, status = self._views(s, out, valid, t_free, status)
        return valid, s.out(end), t_free, status

    def spline_validity(self, ctrl, knots, degree, resolution, threshold=0.0):
        """Sampled check of S clamped B-splines sharing one knot vector (nbk_spline_validity_batch): ctrl (S, n, n_q), knots
        (host) n + degree + 1 values -> valid (S,) bool, t_hit (S,) (the first colliding sample's t, NaN when valid), n_samples
        (S,) int32.  Synchronous: the call reads its sample count back."""
        torch = _require_gpu()
        S, n = self._spline_dims(ctrl)
        kn = _host_f64(knots, n + int(degree) + 1)
        c = _Staged(ctrl, n * self.n_q, "ctrl")
        valid = torch.empty((S,), dtype=torch.uint8, device=c.device)
        t_hit = torch.empty((S,), dtype=torch.float64, device=c.device)
        ns = torch.empty((S,), dtype=torch.int32, device=c.device)
        _lib.check(self._lib.nbk_spline_validity_batch(
            self._h, c.t.data_ptr(), S, n, int(degree), kn.ctypes.data, float(resolution), float(threshold), valid.data_ptr(),
            t_hit.data_ptr(), ns.data_ptr(), self._stream()), "nbk_spline_validity_batch")
        return c.out(valid.bool()), c.out(t_hit), c.out(ns)


    def spline_continuous(self, ctrl, knots, degree, threshold=0.0, max_iter=64, slack=1e-6):
        """Certified continuous check of S clamped B-splines sharing one knot vector (nbk_spline_continuous_batch): ctrl (S, n,
        n_q), knots n + degree + 1 values (copied to the device of ctrl) -> valid (S,) bool, t_free (S,) (how far along [0, 1] the
        trajectory is certified free), status (S,) int32 (``_lib.CA_*``).  Asynchronous on device tensors and capturable."""
        torch = _require_gpu()
        c, kn, S, n = self._stage_splines(ctrl, knots, degree)
        valid = torch.empty((S,), dtype=torch.uint8, device=c.device)
        t_free = torch.empty((S,), dtype=torch.float64, device=c.device)
        status = torch.empty((S,), dtype=torch.int32, device=c.device)
        _lib.check(self._lib.nbk_spline_continuous_batch(
            self._h, c.t.data_ptr(), S, n, int(degree), kn.data_ptr(), float(threshold), int(max_iter), float(slack),
            valid.data_ptr(), t_free.data_ptr(), status.data_ptr(), self._stream()), "nbk_spline_continuous_batch")
        return c.out(valid.bool()), c.out(t_free), c.out(status)

    def _spline_dims(self, ctrl):
        """(S, n) of control points (S, n, n_q), a tensor or anything NumPy takes."""
        shape = tuple(ctrl.shape) if _torch().is_tensor(ctrl) else np.shape(ctrl)
        if len(shape) != 3 or shape[2] != self.n_q:
            raise ValueError(f"control points must have shape (S, n, {self.n_q}), got {shape}")
        return int(shape[0]), int(shape[1])

    def _stage_splines(self, ctrl, knots, degree):
        """The control points and the knots of S splines on one device -> (ctrl ``_Staged``, knots tensor, S, n)."""
        torch = _require_gpu()
        S, n = self._spline_dims(ctrl)
        c = _Staged(ctrl, n * self.n_q, "ctrl")
        if torch.is_tensor(knots):
            kn = knots.to(device=c.device, dtype=torch.float64).contiguous().reshape(-1)
        else:
            kn = torch.from_numpy(_host_f64(knots, n + int(degree) + 1)).to(c.device)
        if kn.numel() != n + int(degree) + 1:
            raise ValueError(f"expected {n + int(degree) + 1} knots, got {kn.numel()}")
        return c, kn, S, n

    @staticmethod
    def _result_triple(torch, out, S, device, names):
        """The result triple of the cloud calls over edges and splines, shape (S,), uint8 / bool, float64 and int32: fresh on
        ``device``, or -- accumulating -- the caller's ``out``, three contiguous CUDA tensors of that form."""
        want = ((torch.uint8, torch.bool), (torch.float64,), (torch.int32,))
        if out is None:
            return tuple(torch.empty((S,), dtype=w[0], device=device) for w in want)
        if not (isinstance(out, (tuple, list)) and len(out) == 3 and
                all(torch.is_tensor(o) and o.is_cuda and o.is_contiguous() and tuple(o.shape) == (S,) and o.dtype in w
                    for o, w in zip(out, want))):
            raise ValueError(f"out must be {names}: contiguous CUDA tensors of shape {(S,)} (uint8 / bool, float64, int32)")
        return tuple(out)

    @staticmethod
    def cloud_spline_workspace_bytes(S: int) -> int:
        return int(_lib.load().nbk_spline_cloud_workspace_bytes(int(S)))

    def cloud_spline_validity(self, cloud, ctrl, knots, degree, resolution, threshold=0.0, shapes=None, out=None, workspace=None):
        """``spline_validity``'s trajectories against ``cloud`` ALONE (a ``PointCloud``; nbk_spline_cloud_validity_batch): a
        trajectory is valid when it is not degenerate and ``cloud_validity`` clears every one of its samples (generated on the
        device, never stored) -> (valid (S,) bool, t_hit (S,) (t of the first colliding sample, NaN when valid), n_samples (S,)
        int32).  The knots are copied to the device of ctrl; the call is asynchronous on device tensors and capturable.
        ``shapes``: as ``cloud_validity``.  ``out``: the CUDA tensors (valid (S,) uint8 / bool, t_hit (S,) float64, n_samples (S,)
        int32) that ``spline_validity`` returned for the same trajectories and resolution: the cloud's verdict is reduced INTO them
        -- an invalid entry stays invalid, only samples before its t_hit are looked at, and t_hit ends as the smaller of the two;
        they are returned.  ``workspace``: optional torch uint8 CUDA tensor of at least ``cloud_spline_workspace_bytes(S)`` bytes;
        by default one is taken from torch's caching allocator (inside a graph capture: from the capture's pool)."""
        torch = _require_gpu()
        c, kn, S, n = self._stage_splines(ctrl, knots, degree)
        bits = self._shape_bits(shapes)
        valid, t_hit, ns = self._result_triple(torch, out, S, c.device, "(valid, t_hit, n_samples)")
        ws, ws_bytes = self._workspace(torch, workspace, self.cloud_spline_workspace_bytes, S, c.device)
        _lib.check(self._lib.nbk_spline_cloud_validity_batch(
            self._h, cloud._h, c.t.data_ptr(), S, n, int(degree), kn.data_ptr(), float(resolution), float(threshold),
            _host_ptr(bits), 0 if out is None else 1, valid.data_ptr(), t_hit.data_ptr(), ns.data_ptr(),
            ws.data_ptr(), ws_bytes, self._stream()), "nbk_spline_cloud_validity_batch")
        return self._views(c, out, valid, t_hit, ns)

    def cloud_spline_continuous(self, cloud, ctrl, knots, degree, threshold=0.0, max_iter=64, slack=1e-6, look_ahead=CLOUD_LOOK_AHEAD,
                                shapes=None, out=None):
        """``spline_continuous``'s trajectories certified against ``cloud`` ALONE (a ``PointCloud``;
        nbk_spline_cloud_continuous_batch): one (trajectory, robot shape) item per lane advances by conservative advancement on the
        shape's clearance from the cloud -> valid (S,) bool, t_free (S,), status (S,) int32 (``_lib.CA_*``).  ``shapes``: as
        ``cloud_validity``; ``look_ahead``: as ``cloud_edge_continuous``.  ``out``: the CUDA tensors (valid (S,) uint8 / bool, t_free
        (S,) float64, status (S,) int32) that ``spline_continuous`` returned for the same trajectories: the cloud's items are reduced
        INTO them -- the result is that of one certified call over the scene's pairs and the cloud together; they are returned."""
        torch = _require_gpu()
        c, kn, S, n = self._stage_splines(ctrl, knots, degree)
        bits = self._shape_bits(shapes)
        valid, t_free, status = self._result_triple(torch, out, S, c.device, "(valid, t_free, status)")
        _lib.check(self._lib.nbk_spline_cloud_continuous_batch(
            self._h, cloud._h, c.t.data_ptr(), S, n, int(degree), kn.data_ptr(), float(threshold), int(max_iter), float(slack),
            float(look_ahead), _host_ptr(bits), 0 if out is None else 1, valid.data_ptr(),
            t_free.data_ptr(), status.data_ptr(), self._stream()), "nbk_spline_cloud_continuous_batch")
        return self._views(c, out, valid, t_free, status)


def held_locals(A, G, L):
    """(H, 3, 4) local poses (A . G) . L_h of held shapes in their holding frame, by the routine the held kernels use
    (nbk_held_locals_host; no GPU needed).  ``A``, ``G``: (4, 4) or (3, 4); ``L``: (H, 4, 4) or (H, 3, 4)."""
    A = np.ascontiguousarray(np.asarray(A, dtype=np.float64)[:3, :4]).reshape(12)
    G = np.ascontiguousarray(np.asarray(G, dtype=np.float64)[:3, :4]).reshape(12)
    L = np.asarray(L, dtype=np.float64)
    L = np.ascontiguousarray(L.reshape(-1, L.shape[-2], 4)[:, :3, :]).reshape(-1, 12)
    out = np.empty_like(L)
    _lib.check(_lib.load().nbk_held_locals_host(A.ctypes.data, G.ctypes.data, L.ctypes.data, L.shape[0], out.ctypes.data),
               "nbk_held_locals_host")
    return out.reshape(-1, 3, 4)


def _held_host_args(model, spec, G):
    """The held arguments of the host twins of the held motion bound (nbk_held_create's, from a ``HeldSpec``) -> (ctypes arguments,
    arrays they point into, K)."""
    S = int(model.n_rshapes)
    A = np.ascontiguousarray(np.asarray(spec.A, dtype=np.float64)[:3, :4]).reshape(12)
    G = np.ascontiguousarray(np.asarray(spec.G if G is None else G, dtype=np.float64)[:3, :4]).reshape(12)
    st = np.ascontiguousarray(spec.shape_type, dtype=np.int32).reshape(-1)
    H = int(st.shape[0])
    L = np.asarray(spec.shape_local, dtype=np.float64)
    L = np.ascontiguousarray(L.reshape(H, L.shape[-2], 4)[:, :3, :]).reshape(H, 12)
    sp = np.ascontiguousarray(spec.shape_param, dtype=np.float64).reshape(H, 4)
    ws = np.ascontiguousarray(sorted(int(w) for w in spec.world_shapes), dtype=np.int32)
    robot = sorted({int(x) for x in spec.robot_shapes})
    bits = None
    if robot:
        bits = np.zeros((max((S + 63) // 64, 1),), dtype=np.uint64)
        for s in robot:
            if not 0 <= s < S:
                raise ValueError(f"robot shape {s} out of range (0..{S - 1})")
            bits[s >> 6] |= np.uint64(1) << np.uint64(s & 63)
    args = (int(spec.frame), A.ctypes.data, G.ctypes.data, H, st.ctypes.data, L.ctypes.data, sp.ctypes.data, int(ws.shape[0]),
            ws.ctypes.data if ws.shape[0] else None, _host_ptr(bits))
    return args, (A, G, st, L, sp, ws, bits), H * (len(robot) + int(ws.shape[0]))


def _held_hull_args(hulls):
    """The hull tables of a held object, (vert_begin, verts, face_begin, planes) as ``HullTable.arrays()`` gives them -> (the five
    ctypes arguments behind nbk_held_create's, arrays they point into)."""
    vb = np.ascontiguousarray(hulls[0], dtype=np.int32).reshape(-1)
    hv = np.ascontiguousarray(hulls[1], dtype=np.float64).reshape(-1, 3)
    fb = np.ascontiguousarray(hulls[2], dtype=np.int32).reshape(-1)
    hp = np.ascontiguousarray(hulls[3], dtype=np.float64).reshape(-1, 4)
    n = int(vb.shape[0]) - 1
    if n < 0 or fb.shape[0] != n + 1 or (n > 0 and (int(vb[n]) != hv.shape[0] or int(fb[n]) != hp.shape[0])):
        raise ValueError("held hull tables: vert_begin / face_begin must have n_hulls + 1 entries that end at the table sizes")
    return (n, vb.ctypes.data, hv.ctypes.data if hv.shape[0] else None, fb.ctypes.data, hp.ctypes.data if hp.shape[0] else None), \
        (vb, hv, fb, hp)


def held_edge_motion_bounds(model, spec, starts, goals, G=None):
    """Motion bounds mu (E, K) of the linear edges starts -> goals for the K items of the held object ``spec`` (a ``HeldSpec``)
    on the SceneModel ``model``, in the items' order: the bits ``edge_motion_bounds`` gives for those pairs on a model that holds
    the held shapes as robot shapes.  The routine nbk_edge_held_continuous_batch advances with, run on the host
    (nbk_edge_held_motion_bounds_host); no GPU needed.  ``G``: the grasp (default: the spec's)."""
    n_q = model.kin.n_q
    s = np.ascontiguousarray(np.asarray(starts, dtype=np.float64)).reshape(-1, n_q)
    g = np.ascontiguousarray(np.asarray(goals, dtype=np.float64)).reshape(-1, n_q)
    if s.shape != g.shape:
        raise ValueError("starts and goals must have the same shape")
    d, keep = model_desc(model)
    args, keep2, K = _held_host_args(model, spec, G)
    mu = np.empty((s.shape[0], K), dtype=np.float64)
    hulls = getattr(spec, "hulls", None)
    if hulls is None:
        _lib.check(_lib.load().nbk_edge_held_motion_bounds_host(C.byref(d), *args, s.ctypes.data, g.ctypes.data, s.shape[0],
                                                                mu.ctypes.data), "nbk_edge_held_motion_bounds_host")
    else:
        hargs, keep3 = _held_hull_args(hulls)
        _lib.check(_lib.load().nbk_edge_held_motion_bounds_hulls_host(C.byref(d), *args, *hargs, s.ctypes.data, g.ctypes.data, s.shape[0],
                                                                      mu.ctypes.data), "nbk_edge_held_motion_bounds_hulls_host")
        del keep3
    del keep, keep2
    return mu


def held_spline_motion_bounds(model, spec, ctrl, knots, degree, G=None):
    """Motion bounds mu (S, n - degree, K) of S clamped B-splines for the K items of the held object ``spec``, per knot span: the bits
    ``spline_motion_bounds`` gives for those pairs on a model that holds the held shapes as robot shapes
    (nbk_spline_held_motion_bounds_host; no GPU needed).  Entries of empty spans are 0."""
    n_q = model.kin.n_q
    c = np.ascontiguousarray(np.asarray(ctrl, dtype=np.float64))
    if c.ndim != 3 or c.shape[2] != n_q:
        raise ValueError(f"control points must have shape (S, n, {n_q}), got {c.shape}")
    S, n = c.shape[:2]
    k = int(degree)
    if not 1 <= k < n:
        raise ValueError("degree must be at least 1 and less than the number of control points")
    kn = _host_f64(knots, n + k + 1)
    d, keep = model_desc(model)
    args, keep2, K = _held_host_args(model, spec, G)
    mu = np.zeros((S, n - k, K), dtype=np.float64)
    hulls = getattr(spec, "hulls", None)
    if hulls is None:
        _lib.check(_lib.load().nbk_spline_held_motion_bounds_host(C.byref(d), *args, c.ctypes.data, S, n, k, kn.ctypes.data,
                                                                  mu.ctypes.data), "nbk_spline_held_motion_bounds_host")
    else:
        hargs, keep3 = _held_hull_args(hulls)
        _lib.check(_lib.load().nbk_spline_held_motion_bounds_hulls_host(C.byref(d), *args, *hargs, c.ctypes.data, S, n, k, kn.ctypes.data,
                                                                        mu.ctypes.data), "nbk_spline_held_motion_bounds_hulls_host")
        del keep3
    del keep, keep2
    return mu


def held_edge_shape_motion_bounds(model, spec, starts, goals, G=None, hulls=False):
    """Motion bounds mu (E, H) of the linear edges starts -> goals for the H shapes of the held object ``spec`` (a ``HeldSpec``) on
    the SceneModel ``model``, every joint of the holding path counting: the bits ``edge_shape_motion_bounds`` gives for robot shapes
    S .. S+H-1 on a model that holds the held shapes as robot shapes.  The routine nbk_edge_held_cloud_continuous_batch advances
    with, run on the host (nbk_edge_held_shape_motion_bounds_host); no GPU needed.  ``G``: the grasp (default: the spec's).
    ``hulls=True``: the spec's hull tables go along (nbk_edge_held_shape_motion_bounds_hulls_host); without it a spec that holds a
    hull shape is refused, as the held-versus-cloud entries refuse an object that was not opted in."""
    n_q = model.kin.n_q
    s = np.ascontiguousarray(np.asarray(starts, dtype=np.float64)).reshape(-1, n_q)
    g = np.ascontiguousarray(np.asarray(goals, dtype=np.float64)).reshape(-1, n_q)
    if s.shape != g.shape:
        raise ValueError("starts and goals must have the same shape")
    d, keep = model_desc(model)
    args, keep2, _ = _held_host_args(model, spec, G)
    H = args[3]
    mu = np.empty((s.shape[0], H), dtype=np.float64)
    tables = getattr(spec, "hulls", None) if hulls else None
    if tables is None:
        _lib.check(_lib.load().nbk_edge_held_shape_motion_bounds_host(C.byref(d), *args[:7], s.ctypes.data, g.ctypes.data, s.shape[0],
                                                                      mu.ctypes.data), "nbk_edge_held_shape_motion_bounds_host")
    else:
        hargs, keep3 = _held_hull_args(tables)
        _lib.check(_lib.load().nbk_edge_held_shape_motion_bounds_hulls_host(C.byref(d), *args[:7], *hargs, s.ctypes.data, g.ctypes.data,
                                                                            s.shape[0], mu.ctypes.data),
                   "nbk_edge_held_shape_motion_bounds_hulls_host")
        del keep3
    del keep, keep2
    return mu


def held_spline_shape_motion_bounds(model, spec, ctrl, knots, degree, G=None, hulls=False):
    """Motion bounds mu (S, n - degree, H) of S clamped B-splines for the H shapes of the held object ``spec``, per knot span: the
    bits ``spline_shape_motion_bounds`` gives for robot shapes S .. S+H-1 on a model that holds the held shapes as robot shapes
    (nbk_spline_held_shape_motion_bounds_host; no GPU needed).  Entries of empty spans are 0.  ``hulls``: as
    ``held_edge_shape_motion_bounds`` (nbk_spline_held_shape_motion_bounds_hulls_host)."""
    n_q = model.kin.n_q
    c = np.ascontiguousarray(np.asarray(ctrl, dtype=np.float64))
    if c.ndim != 3 or c.shape[2] != n_q:
        raise ValueError(f"control points must have shape (S, n, {n_q}), got {c.shape}")
    S, n = c.shape[:2]
    k = int(degree)
    if not 1 <= k < n:
        raise ValueError("degree must be at least 1 and less than the number of control points")
    kn = _host_f64(knots, n + k + 1)
    d, keep = model_desc(model)
    args, keep2, _ = _held_host_args(model, spec, G)
    H = args[3]
    mu = np.zeros((S, n - k, H), dtype=np.float64)
    tables = getattr(spec, "hulls", None) if hulls else None
    if tables is None:
        _lib.check(_lib.load().nbk_spline_held_shape_motion_bounds_host(C.byref(d), *args[:7], c.ctypes.data, S, n, k, kn.ctypes.data,
                                                                        mu.ctypes.data), "nbk_spline_held_shape_motion_bounds_host")
    else:
        hargs, keep3 = _held_hull_args(tables)
        _lib.check(_lib.load().nbk_spline_held_shape_motion_bounds_hulls_host(C.byref(d), *args[:7], *hargs, c.ctypes.data, S, n, k,
                                                                              kn.ctypes.data, mu.ctypes.data),
                   "nbk_spline_held_shape_motion_bounds_hulls_host")
        del keep3
    del keep, keep2
    return mu


class DeviceHeld:
    """A held object on the device (nbk_held): H shapes riding on moving frame ``frame`` of ``dev``'s descriptor, with the world
    shapes and robot shapes (``SceneModel`` order) its verdict looks at.  ``A``: the link's constant pose in the frame, ``G``: the
    default grasp, ``shape_local`` (H, 4, 4) / (H, 3, 4): each shape in the object's frame; ``shape_type`` / ``shape_param``: as a
    robot shape's.  ``hulls``: the hull tables (vert_begin, verts, face_begin, planes) of held SH_HULL shapes -- given, the object is
    made by nbk_held_create_hulls; without them a hull shape is refused.  ``scans=True``: the held-versus-cloud calls serve the
    object's hulls too (nbk_held_set_cloud_hulls, set once here; ``sees_scans``); without it they refuse an object that holds one.
    Allocated once; the descriptor is kept alive."""

    def __init__(self, dev, frame, A, G, shape_type, shape_local, shape_param, world_shapes=(), robot_shapes=(), hulls=None, scans=False):
        _require_gpu()
        if dev.scene is None:
            raise ValueError("a held object needs a descriptor made from a SceneModel")
        A = np.ascontiguousarray(np.asarray(A, dtype=np.float64)[:3, :4]).reshape(12)
        G = np.ascontiguousarray(np.asarray(G, dtype=np.float64)[:3, :4]).reshape(12)
        st = np.ascontiguousarray(shape_type, dtype=np.int32).reshape(-1)
        H = int(st.shape[0])
        L = np.asarray(shape_local, dtype=np.float64)
        L = np.ascontiguousarray(L.reshape(H, L.shape[-2], 4)[:, :3, :]).reshape(H, 12)
        sp = np.ascontiguousarray(shape_param, dtype=np.float64).reshape(H, 4)
        ws = np.ascontiguousarray(sorted(int(w) for w in world_shapes), dtype=np.int32)
        robot = [int(x) for x in robot_shapes]
        bits = dev._shape_bits(robot) if robot else None
        h = C.c_void_p()
        args = (dev._h, int(frame), A.ctypes.data, G.ctypes.data, H, st.ctypes.data, L.ctypes.data, sp.ctypes.data, int(ws.shape[0]),
                ws.ctypes.data if ws.shape[0] else None, _host_ptr(bits))
        if hulls is None:
            _lib.check(dev._lib.nbk_held_create(*args, C.byref(h)), "nbk_held_create")
        else:
            hargs, keep = _held_hull_args(hulls)
            _lib.check(dev._lib.nbk_held_create_hulls(*args, *hargs, C.byref(h)), "nbk_held_create_hulls")
            del keep
        self._h, self._lib, self.dev, self.n_shapes = h, dev._lib, dev, H
        self.has_hull = bool(np.any(st == 5))           # (the held-versus-cloud entries refuse such an object unless it sees scans)
        self.sees_scans = bool(scans)
        if self.sees_scans:
            _lib.check(dev._lib.nbk_held_set_cloud_hulls(h, 1), "nbk_held_set_cloud_hulls")
        self.n_items = int(dev._lib.nbk_held_item_count(h))

    def items(self):
        """(K, 3) int32: (held shape, kind -- 0 robot shape, 1 world shape --, index in ``SceneModel`` order) of the items, the
        columns of ``DeviceModel.held_distances`` (nbk_held_items)."""
        out = np.zeros((self.n_items, 3), dtype=np.int32)
        _lib.check(self._lib.nbk_held_items(self._h, out.ctypes.data if self.n_items else None), "nbk_held_items")
        return out

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                self._lib.nbk_held_destroy(h)
            except Exception:
                pass
            self._h = None


def selftest_math(a, b):
    """sincos(a), sqrt(a), a/b as the kernels compute them (arithmetic-contract check)."""
    torch = _require_gpu()
    lib = _lib.load()
    ta = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    tb = torch.from_numpy(np.ascontiguousarray(b, dtype=np.float64)).cuda()
    outs = [torch.empty_like(ta) for _ in range(4)]
    _lib.check(lib.nbk_selftest_math(ta.data_ptr(), tb.data_ptr(), ta.numel(), *[o.data_ptr() for o in outs],
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)), "nbk_selftest_math")
    return [o.cpu().numpy() for o in outs]


def knn_prefix_device(points, k):
    """(N, d) float32 -> (N, k) int64 neighbour lists among the points inserted before (nbk_knn_prefix), -1 padded."""
    torch = _require_gpu()
    lib = _lib.load()
    x = np.ascontiguousarray(points, dtype=np.float32)
    n, dim = x.shape
    t = torch.from_numpy(x).cuda()
    out = torch.empty((n, k), dtype=torch.int32, device="cuda")
    _lib.check(lib.nbk_knn_prefix(t.data_ptr(), n, dim, int(k), out.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "nbk_knn_prefix")
    return out.cpu().numpy().astype(np.int64)
