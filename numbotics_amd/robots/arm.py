"""``Arm``: the reference's robot front-end (numbotics/robots/arm.py) over the MI355X engine.

Same method names, argument order, defaults and exception types as upstream.  What changes:

  * ``forward_kinematics`` / ``jacobian`` run as HIP kernels (one configuration per lane) instead of
    serial numba loops (robots/helpers.py:91-187); they accept NumPy arrays or torch CUDA tensors.
  * ``in_collision`` / ``closest_to`` / ``collisions`` no longer push one ``q`` at a time through
    PyBullet (arm.py:555-604, physics/chain.py:944-969): the allowed pairs are compiled once into a
    device descriptor and whole batches are checked per launch.  ``in_collision`` additionally accepts
    ``(B, dof)`` input and then returns ``(B,)`` bool; the ``(dof,)`` form returns a Python bool as
    upstream.
  * Reference quirks: Q1 -- FK/Jacobian here are correct for every link, upstream
    only for frames that end in a FIXED joint; Q2 -- ``global_pose=False`` is treated as ``None``;
    Q3 -- the default self-collision rule is upstream's *effective* one (all non-adjacent shaped
    pairs); ``weld_filter=True`` enables the rule upstream intended.
"""
import contextlib

import numpy as np
import networkx as nx

from numbotics_amd.physics import Chain, Constraint, Link, PhysicsObject, Proximity
from numbotics_amd.utils import Shape, logger
from .robot import Robot
from .model import compile_kinematics, compile_scene


def _is_tensor(x):
    return type(x).__module__.startswith("torch")


class Arm(Robot):

    def __init__(self, chain, weld_filter: bool = False, compound: bool = True, bullet_margins: bool = True,
                 movable_world: bool = False, world_radius=None):
        """``bullet_margins`` (additive, default True): every box / cylinder / mesh hull that has no explicit ``collision_margin``
        gets the margin Bullet itself applies to the shapes ``pybullet.createCollisionShape`` builds for the reference
        (numbotics/utils/shape.py:60-109; robots/model.py ``bullet_margin``: boxes / cylinders are rounded by
        min(0.04, a tenth of the smallest half extent), hulls inflated by 0.001) -- the restatement closest to the reference's
        ``getClosestPoints`` answers.  ``False`` = the sharp analytic shapes (margin 0); can be switched later through the
        ``bullet_margins`` property.

        ``movable_world`` (additive, default False): keep the device scene when a world change moved obstacles only --
        ``obj.pose = T``, ``cube.position = p``, another chain's ``configuration = q``.  The (small) SceneModel is still recompiled
        on the host, but when everything except the world shapes' poses is unchanged the new poses are written into the existing
        descriptor on the device (``DeviceModel.set_world_poses``) in stream order: no descriptor build, no scratch reallocation,
        captured graphs and cached IRIS bisection graphs stay valid.  Any other change (an object added or removed, a shape resized,
        a plane turned, pair edits, ``bullet_margins``) rebuilds as without the flag, and so does a centre that leaves
        ``world_radius`` -- how far from the world origin an obstacle's shape centre may go; default
        ``robots.model.default_world_radius``: twice the larger of the arm's reach and the farthest obstacle centre of the scene
        the descriptor is built from.  A generous radius costs a little broadphase precision, never a result."""
        super().__init__(chain)
        self._movable_world = bool(movable_world)
        if world_radius is not None:
            world_radius = float(world_radius)
            if not self._movable_world:
                raise ValueError("world_radius is meaningful with movable_world=True only")
            if not (0.0 <= world_radius < np.inf):
                raise ValueError(f"world_radius must be finite and >= 0, got {world_radius}")
        self._world_radius = world_radius
        self._movable_dev = None       # (structure signature, DeviceModel) of the movable device scene
        self._weld_filter = weld_filter
        self._compound = compound
        self._bullet_margins = bool(bullet_margins)
        self._kin = compile_kinematics(chain)
        # per-frame flattened sequences in the reference's own format (arm.py:61), kept for inspection
        self._link_joint_sequence = {}
        self._links_from_nodes = {}
        root = next(iter(nx.topological_sort(chain._G)))
        for node in chain._G.nodes:
            self._links_from_nodes[node] = chain._G.nodes[node]["link"]
            fr = self._kin.frames[node]
            if node == root:
                self._link_joint_sequence[node] = tuple()
                continue
            offs = [self._T44(self._kin.joint_offset[k]) for k in fr.path]
            if fr.trailing_fixed:
                offs.append(fr.local)
            self._link_joint_sequence[node] = (
                np.array(offs).reshape(-1, 4, 4),
                self._kin.joint_axis[fr.path].reshape(-1, 3),
                np.array([0 if self._kin.joint_type[k] == 0 else 1 for k in fr.path], dtype=np.int64),
                self._kin.joint_qidx[fr.path].astype(np.int64),
            )
        self._additional_self_collision_pairs = set()
        self._void_self_collision_pairs = set()
        self._additional_collision_pairs = set()
        self._void_collision_pairs = set()
        self._pairs_version = 0
        self._kin_dev = None
        self._scene_cache = None       # (key, SceneModel, DeviceModel)
        self._retired_dev = None
        self.self_collision_pairs()

    @staticmethod
    def _T44(p12):
        T = np.eye(4)
        T[:3, :4] = np.asarray(p12).reshape(3, 4)
        return T

    # ---- passthrough properties (arm.py:73-124) ----------------------------------------------------
    @property
    def base_pose(self):
        return self._chain.base_pose

    @property
    def joint_limits(self):
        return self._chain.joint_limits

    @property
    def dof(self):
        return self._chain.dof

    @property
    def configuration(self):
        return self._chain.configuration

    @configuration.setter
    def configuration(self, q):
        self._chain.configuration = q

    @contextlib.contextmanager
    def stateless(self):
        """Upstream saves/restores PyBullet state around a query (arm.py:128-146); queries here are pure."""
        yield

    @contextlib.contextmanager
    def pool(self, poolsize: int = 1):
        """Upstream clones the world per CPU thread (arm.py:149-187).  The device path batches instead;
        the engine is re-entrant, so the pool is ``poolsize`` references to this Arm."""
        yield tuple(self for _ in range(poolsize))

    # ---- collision pair bookkeeping (arm.py:190-366) -----------------------------------------------
    def _in_chain(self, x):
        return isinstance(x, Link) and x._body_id == self._chain._pyb_id and x._world_name == self._chain._world_name

    def self_collision_pairs(self):
        if not hasattr(self, '_self_collision_pairs'):
            pairs = set()
            G_u = self._chain._G.to_undirected()
            shaped = [l for l in self._chain._links if l._collision_shape.shape != Shape.EMPTY]
            for a in shaped:
                for b in shaped:
                    if a is b:
                        continue
                    if self._weld_filter:
                        path = nx.shortest_path(G_u, a._name, b._name)
                        moving = sum(1 for u, v in zip(path[:-1], path[1:])
                                     if G_u.edges[(u, v)]["joint"].type != Constraint.FIXED)
                        if moving < 2:
                            continue
                    if not G_u.has_edge(a._name, b._name) and (b, a) not in pairs:
                        pairs.add((a, b))
            self._self_collision_pairs = pairs
        return self._self_collision_pairs.union(self._additional_self_collision_pairs).difference(
            self._void_self_collision_pairs)

    def collision_pairs(self):
        pairs = set()
        for link in self._chain._links:
            if link._collision_shape.shape == Shape.EMPTY:
                continue
            for obj in self._chain.world.objects():
                if obj == self._chain:
                    continue
                if isinstance(obj, PhysicsObject):
                    if obj._collision_shape.shape == Shape.EMPTY:
                        continue
                    pairs.add((link, obj))
                elif isinstance(obj, Chain):
                    for other in obj._links:
                        pairs.add((link, other))
        return pairs.union(self.self_collision_pairs()).union(self._additional_collision_pairs).difference(
            self._void_collision_pairs)

    def _resolve(self, x):
        if isinstance(x, str):
            found = self._links_from_nodes.get(x)
            if found is None:
                found = self._chain.world.get_object(x)
                if found is None:
                    raise ValueError(f"Object name: {x} must be a valid object in the world")
            return found
        return x

    def _ordered(self, link_a, link_b, verb):
        link_a, link_b = self._resolve(link_a), self._resolve(link_b)
        a_in, b_in = self._in_chain(link_a), self._in_chain(link_b)
        if not a_in and not b_in:
            logger.warning(f"Did not {verb} collision pair between {link_a.name} and {link_b.name} "
                           "because neither is in the chain")
            return None
        if not a_in:
            link_a, link_b = link_b, link_a
            b_in = False
        return link_a, link_b, b_in

    @staticmethod
    def _has(pairs, a, b):
        return (a, b) in pairs or (b, a) in pairs

    @staticmethod
    def _drop(pairs, a, b):
        if (a, b) in pairs:
            pairs.remove((a, b))
        elif (b, a) in pairs:
            pairs.remove((b, a))

    def add_collision_pair(self, link_a, link_b):
        r = self._ordered(link_a, link_b, "add")
        if r is None:
            return
        a, b, is_self = r
        if is_self:
            if self._has(self.self_collision_pairs(), a, b):
                logger.warning(f"Did not add collision pair between {a.name} and {b.name} because it is "
                               "already a self collision pair")
            else:
                # upstream files this under _additional_collision_pairs, where its own self-collision
                # filter (arm.py:569-572) never looks; here the pair becomes active
                self._additional_self_collision_pairs.add((a, b))
            self._drop(self._void_self_collision_pairs, a, b)
        else:
            if self._has(self.collision_pairs(), a, b):
                logger.warning(f"Did not add collision pair between {a.name} and {b.name} because it is "
                               "already a collision pair")
            else:
                self._additional_collision_pairs.add((a, b))
            self._drop(self._void_collision_pairs, a, b)
        self._pairs_version += 1

    def remove_collision_pair(self, link_a, link_b):
        r = self._ordered(link_a, link_b, "remove")
        if r is None:
            return
        a, b, is_self = r
        if is_self:
            self._drop(self._additional_self_collision_pairs, a, b)
            if self._has(self._void_self_collision_pairs, a, b):
                logger.warning(f"Did not remove collision pair between {a.name} and {b.name} because it is "
                               "has already been removed")
            elif (a, b) in self.self_collision_pairs():
                self._void_self_collision_pairs.add((a, b))
            elif (b, a) in self.self_collision_pairs():
                self._void_self_collision_pairs.add((b, a))
        else:
            self._drop(self._additional_collision_pairs, a, b)
            if self._has(self._void_collision_pairs, a, b):
                logger.warning(f"Did not remove collision pair between {a.name} and {b.name} because it is "
                               "has already been removed")
            elif (a, b) in self.collision_pairs():
                self._void_collision_pairs.add((a, b))
            elif (b, a) in self.collision_pairs():
                self._void_collision_pairs.add((b, a))
        self._pairs_version += 1

    # ---- descriptors ----------------------------------------------------------------------------------
    def _sorted_pairs(self, pairs):
        order = {l._name: i for i, l in enumerate(self._chain._links)}

        def key(p):
            a, b = p
            if not self._in_chain(a):
                a, b = b, a
            kb = (0, order[b._name]) if self._in_chain(b) else (1, b.name)
            return (order[a._name], kb)
        return sorted(pairs, key=key)

    @property
    def bullet_margins(self) -> bool:
        return self._bullet_margins

    @bullet_margins.setter
    def bullet_margins(self, on: bool):
        self._bullet_margins = bool(on)
        self._retire_scene_cache()
        self._scene_cache = None

    def _retire_scene_cache(self):
        """Keep the outgoing device scene alive until its successor exists (``_scene_device`` drops it then).  Freed first, its
        handle can come straight back from the allocator for the new descriptor, and a caller that compares handles across a
        rebuild (tests/test_broad_spec.py does) would take the new scene for the old one.  The old scratch goes before the
        new descriptor allocates any of its own."""
        if self._scene_cache is not None and self._scene_cache[2] is not None:
            self._retired_dev = self._scene_cache[2]

    def scene_model(self, pairs=None):
        """The flat SceneModel (robots/model.py) of the current world and pair set."""
        if pairs is not None:
            return compile_scene(self._chain, self._refreshed_kin(), self._sorted_pairs(pairs), self._compound, self._bullet_margins)
        key = (self._chain.world._revision, self._pairs_version, self._bullet_margins)
        if self._scene_cache is None or self._scene_cache[0] != key:
            sm = compile_scene(self._chain, self._refreshed_kin(), self._sorted_pairs(self.collision_pairs()),
                               self._compound, self._bullet_margins)
            self._retire_scene_cache()
            self._scene_cache = (key, sm, None)
        return self._scene_cache[1]

    def _refreshed_kin(self):
        bp = np.ascontiguousarray(self._chain.base_pose[:3, :4]).reshape(12)
        if not np.array_equal(bp, self._kin.base_pose):
            self._kin.base_pose = bp
            self._kin_dev = None
        return self._kin

    def _kin_device(self):
        from numbotics_amd.engine import DeviceModel
        self._refreshed_kin()
        if self._kin_dev is None:
            self._kin_dev = DeviceModel(self._kin)
        return self._kin_dev

    def _scene_device(self):
        from numbotics_amd.engine import DeviceModel
        sm = self.scene_model()
        key, _, dev = self._scene_cache
        if dev is None:
            if self._movable_world:
                dev = self._moved_scene_device(sm, DeviceModel)
            else:
                dev = DeviceModel(sm)
            self._scene_cache = (key, sm, dev)
            self._retired_dev = None
        return sm, dev

    def _moved_scene_device(self, sm, DeviceModel):
        """The movable device scene for the freshly compiled ``sm``: the existing descriptor with ``sm``'s world poses when only
        poses changed and every centre is inside its radius, a new one otherwise."""
        sig = sm.structure_signature()
        if self._movable_dev is not None and self._movable_dev[0] == sig:
            dev = self._movable_dev[1]
            centres = sm.wshape_pose.reshape(-1, 3, 4)[:, :, 3]
            if np.all(np.isfinite(sm.wshape_pose)) and (sm.n_wshapes == 0 or float(np.max(np.linalg.norm(centres, axis=1))) <= dev.world_radius):
                dev.set_world_poses(sm.wshape_pose, stream_ordered=True)
                dev.scene = sm
                return dev
        dev = DeviceModel(sm, movable=True, world_radius=self._world_radius)
        self._movable_dev = (sig, dev)
        return dev

    # ---- moving obstacles from device data ---------------------------------------------------------------
    def set_obstacle_poses(self, poses):
        """Move the obstacles from DEVICE data (perception output, graph replay; ``movable_world=True`` only): ``poses`` a float64
        CUDA tensor (W, 3, 4) or (W, 12), the world pose of every world SHAPE in ``scene_model()`` order -- rows
        ``obstacle_shape_index(obj)`` belong to ``obj``; a caller that holds body poses forms ``body_pose @ local`` on the device
        with ``obstacle_shape_locals()``.  Issued on the current stream (capturable); it does not touch the Python objects'
        ``pose``.  When both ways are used, the one applied last wins: these poses hold until the next world change made through
        the Python objects (which writes THEIR poses for every shape), and the other way round."""
        if not self._movable_world:
            raise ValueError("set_obstacle_poses needs an Arm made with movable_world=True")
        _, dev = self._scene_device()
        dev.set_world_poses(poses)

    def obstacle_shape_index(self, obj):
        """Rows of ``set_obstacle_poses`` (world shapes of ``scene_model()``) that belong to ``obj`` (an object, a link of another
        chain, or its name)."""
        obj = self._resolve(obj)
        sm = self.scene_model()
        return np.array([w for w in range(sm.n_wshapes) if sm.objects[sm.wshape_obj[w]] is obj], dtype=np.int64)

    def obstacle_shape_locals(self):
        """(W, 4, 4) constant shape-in-body transforms of the world shapes (``robots.model.scene_shape_locals``)."""
        from .model import scene_shape_locals
        return scene_shape_locals(self.scene_model(), self._compound, self._bullet_margins)

    # ---- kinematics -----------------------------------------------------------------------------------
    def _check_frame_q(self, q, frame):
        if frame not in self._kin.frames:
            raise ValueError(f"Frame {frame} not found in chain")
        if q.shape[-1] != self.dof:
            raise ValueError(f"q must have {self.dof} elements")

    @staticmethod
    def _reshape(x, shape):
        return x.reshape(shape)

    def _pose_arg(self, pose, q_shape, name):
        """-> (single 4x4 ndarray | None, batched (B,4,4) | None)"""
        if pose is None:
            return None, None
        if tuple(pose.shape[-2:]) != (4, 4):
            raise ValueError(f"{name} must be a 4x4 matrix")
        if pose.ndim == 2:
            single = pose.detach().cpu().numpy() if _is_tensor(pose) else np.asarray(pose, dtype=np.float64)
            return single, None
        if tuple(pose.shape[:-2]) != tuple(q_shape[:-1]):
            raise ValueError(f"{name} must have the same batch dimensions as q")
        return None, pose.reshape(-1, 4, 4)

    def forward_kinematics(self, q, frame: str, use_com: bool = False, local_pose=None):
        self._check_frame_q(q, frame)
        shape = tuple(q.shape)
        single, batched = self._pose_arg(local_pose, shape, "local_pose")
        extra = None
        if use_com:
            extra = self._links_from_nodes[frame]._offset
        if single is not None:
            extra = single if extra is None else extra @ single
        T = self._kin_device().fk(q.reshape(-1, self.dof), frame, extra_local=extra, local_pose=batched)
        if len(shape) == 1:
            return T[0]
        return T.reshape(*shape[:-1], 4, 4)

    def forward_kinematics_all(self, q, frames=None, use_com: bool = False):
        """Poses of many links in one launch (additive; upstream loops ``forward_kinematics`` over the link names):
        ``(..., dof)`` -> ``(..., L, 4, 4)`` and the list of frame names (default: every link of the chain, chain order).
        Each pose is bit-identical to ``forward_kinematics(q, name, use_com)``."""
        if q.shape[-1] != self.dof:
            raise ValueError(f"q must have {self.dof} elements")
        names = list(self._kin.frames.keys()) if frames is None else list(frames)
        for f in names:
            if f not in self._kin.frames:
                raise ValueError(f"Frame {f} not found in chain")
        extra = {f: self._links_from_nodes[f]._offset for f in names} if use_com else None
        shape = tuple(q.shape)
        T = self._kin_device().fk_frames(q.reshape(-1, self.dof), names, extra_locals=extra)
        if len(shape) == 1:
            return T[0], names
        return T.reshape(*shape[:-1], len(names), 4, 4), names

    def jacobian(self, q, frame: str, use_com: bool = False, local_pose=None, global_pose=False):
        self._check_frame_q(q, frame)
        if global_pose is False:          # upstream's default crashes on `.shape` (App. A Q2)
            global_pose = None
        shape = tuple(q.shape)
        if global_pose is not None and local_pose is not None:
            raise ValueError("local_pose and global_pose cannot both be provided")
        l_single, l_batched = self._pose_arg(local_pose, shape, "local_pose")
        g_single, g_batched = self._pose_arg(global_pose, shape, "global_pose")
        q2 = q.reshape(-1, self.dof)
        B = q2.shape[0]
        extra = self._links_from_nodes[frame]._offset if use_com else None
        if l_single is not None:
            extra = l_single if extra is None else extra @ l_single
        if g_single is not None:
            g_batched = np.tile(g_single[None], (B, 1, 1))
        if len(self._kin.frames[frame].path) == 0:
            J = np.zeros((B, 6, self.dof))      # arm.py:455-457
            if _is_tensor(q):
                import torch
                J = torch.zeros((B, 6, self.dof), dtype=torch.float64, device=q.device)
        else:
            J = self._kin_device().jacobian(q2, frame, extra_local=extra, local_pose=l_batched, global_pose=g_batched)
        if len(shape) == 1:
            return J[0]
        return J.reshape(*shape[:-1], 6, self.dof)

    def inverse_kinematics(self, pose, q0, frame: str, use_com: bool = False, use_limits: bool = False,
                           tol: float = 1e-6, max_iter: int = 100, max_failures: int = 15):
        """Damped-least-squares IK, signature and return shapes of upstream (arm.py:464-552): ``(success, q)`` with
        ``success`` a flat bool array and ``q`` shaped ``(dof,)`` or ``(*batch_dims, dof)``.  All problems iterate
        inside one launch (``nbk_ik_batch``).  Upstream's own loop cannot run (its ``jacobian`` call hits Q2); the
        per-element arithmetic it writes down is what the kernel follows, with a Cholesky solve for LAPACK's LU."""
        if frame not in self._kin.frames:
            raise ValueError(f"Frame {frame} not found in chain")
        if q0.shape[-1] != self.dof:
            raise ValueError(f"q0 must have {self.dof} elements")
        if max_iter < 1:
            raise ValueError("max_iter must be greater than 0")
        if tuple(pose.shape[-2:]) != (4, 4):
            raise ValueError("pose must be a 4x4 matrix")
        batch_dims = None
        if pose.ndim > 2:
            batch_dims = tuple(pose.shape[:-2])
            pose = pose.reshape(-1, 4, 4)
        if q0.ndim > 1:
            if batch_dims:
                if tuple(q0.shape[:-1]) != batch_dims:
                    raise ValueError("pose and q0 must have the same batch dimensions")
            else:
                batch_dims = tuple(q0.shape[:-1])
        q0f = q0.reshape(-1, self.dof)
        posef = pose.reshape(-1, 4, 4)
        n = max(int(q0f.shape[0]), int(posef.shape[0]))
        if _is_tensor(q0f) or _is_tensor(posef):
            import torch
            q0f = q0f if _is_tensor(q0f) else torch.from_numpy(np.ascontiguousarray(q0f, dtype=np.float64))
            posef = posef if _is_tensor(posef) else torch.from_numpy(np.ascontiguousarray(posef, dtype=np.float64))
            if q0f.shape[0] != n:
                q0f = q0f.expand(n, self.dof)
            if posef.shape[0] != n:
                posef = posef.expand(n, 4, 4)
            q0f, posef = q0f.cuda(), posef.cuda()
        else:
            if q0f.shape[0] != n:
                q0f = np.tile(q0f, (n, 1))
            if posef.shape[0] != n:
                posef = np.tile(posef, (n, 1, 1))
        extra = self._links_from_nodes[frame]._offset if use_com else None
        limits = np.ascontiguousarray(self.joint_limits, dtype=np.float64) if use_limits else None
        ok, q, _, _ = self._kin_device().ik(posef, q0f, frame, extra_local=extra, limits=limits, tol=tol,
                                            max_iter=max_iter, max_failures=max_failures)
        if batch_dims is None:
            return ok, q[0]
        return ok, q.reshape(*batch_dims, self.dof)

    # ---- collision queries ------------------------------------------------------------------------------
    def _proximities(self, sm, pairs, dist, wit):
        """Proximity records of the given pair indices from their (S,) distances and (S, 9) witnesses."""
        out = []
        for i, p in enumerate(pairs):
            subj, targ = sm.pair_members(p)
            out.append(Proximity(subject=subj, target=targ, position_on_subject=wit[i, 0:3].copy(),
                                 position_on_target=wit[i, 3:6].copy(), normal_target_to_subject=wit[i, 6:9].copy(),
                                 distance=float(dist[i])))
        return out

    def collisions(self, q):
        """One Proximity per allowed primitive pair (compound links contribute one per element pair)."""
        if tuple(q.shape) != (self.dof,):
            raise ValueError(f"q must be a 1D array with {self.dof} elements")
        sm, dev = self._scene_device()
        if sm.n_pairs == 0:
            return []
        qn = q.detach().cpu().numpy() if _is_tensor(q) else np.asarray(q, dtype=np.float64)
        dist, wit = dev.pair_distances(qn.reshape(1, -1), witness=True)
        return self._proximities(sm, range(sm.n_pairs), dist[0], wit[0])

    def self_collisions(self, q):
        if tuple(q.shape) != (self.dof,):
            raise ValueError(f"q must be a 1D array with {self.dof} elements")
        return [p for p in self.collisions(q) if self._in_chain(p.target)
                and self._has(self.self_collision_pairs(), p.subject, p.target)]

    def closest_to(self, q):
        """``min(collisions(q), key=distance)`` (arm.py:599-600) without building the other Proximity records."""
        if tuple(q.shape) != (self.dof,):
            raise ValueError(f"q must be a 1D array with {self.dof} elements")
        sm, dev = self._scene_device()
        if sm.n_pairs == 0:
            raise ValueError("min() arg is an empty sequence")
        qn = q.detach().cpu().numpy() if _is_tensor(q) else np.asarray(q, dtype=np.float64)
        dist, wit = dev.pair_distances(qn.reshape(1, -1), witness=True)
        p = int(np.argmin(dist[0]))                       # first minimum, as min() over the list
        subj, targ = sm.pair_members(p)
        return Proximity(subject=subj, target=targ, position_on_subject=wit[0, p, 0:3].copy(),
                         position_on_target=wit[0, p, 3:6].copy(), normal_target_to_subject=wit[0, p, 6:9].copy(),
                         distance=float(dist[0, p]))

    def in_collision(self, q, threshold: float = 0.0):
        """``(dof,)`` -> bool as upstream (arm.py:603-604); ``(..., dof)`` -> bool array/tensor (additive)."""
        if q.shape[-1] != self.dof:
            raise ValueError(f"q must have {self.dof} elements")
        sm, dev = self._scene_device()
        if q.ndim == 1:
            if sm.n_pairs == 0:
                raise ValueError("min() arg is an empty sequence")       # what upstream's closest_to raises
            if isinstance(q, np.ndarray):
                return dev.validity_scalar(q, threshold)                 # host fast path: pinned staging, one wait
            return bool(dev.validity(q.reshape(1, -1), threshold)[0])
        mask = dev.validity(q.reshape(-1, self.dof), threshold)
        return mask.reshape(tuple(q.shape[:-1]))

    # ---- point-cloud obstacles ---------------------------------------------------------------------------
    def _cloud_shapes(self, sm, ignore_links):
        """Robot shape indices of ``sm`` without the shapes of ``ignore_links`` (Link objects or link names); None = all."""
        names = {getattr(l, "_name", l) for l in ignore_links}
        if not names:
            return None
        known = {l._name for l in sm.links}
        for n in names:
            if n not in known:
                raise ValueError(f"Link {n} not found in chain")
        return [s for s in range(sm.n_rshapes) if sm.links[sm.rshape_link[s]]._name not in names]

    def in_collision_with_cloud(self, q, cloud, threshold: float = 0.0, ignore_links=()):
        """Is the arm closer than ``threshold`` to a point of ``cloud`` (``numbotics_amd.physics.PointCloud``: every point a sphere
        of the cloud's radius)?  ``(dof,)`` -> bool, ``(..., dof)`` -> bool array / tensor, like ``in_collision``.  This is the
        cloud's verdict ONLY -- self-collision and the world's objects are ``in_collision``'s; full validity is
        ``arm.in_collision(q) | arm.in_collision_with_cloud(q, cloud)``.  ``ignore_links``: links (or their names) whose shapes are
        left out, e.g. the base standing on a scanned table."""
        if q.shape[-1] != self.dof:
            raise ValueError(f"q must have {self.dof} elements")
        sm, dev = self._scene_device()
        shapes = self._cloud_shapes(sm, ignore_links)
        if q.ndim == 1:
            return bool(dev.cloud_validity(cloud, q.reshape(1, -1), threshold, shapes=shapes)[0])
        mask = dev.cloud_validity(cloud, q.reshape(-1, self.dof), threshold, shapes=shapes)
        return mask.reshape(tuple(q.shape[:-1]))

    # ---- held objects ----------------------------------------------------------------------------------------
    def attach(self, obj, link, pose=None, touch_links=(), meshes=False, mesh_scans=False):
        """Put ``obj`` (a ``PhysicsObject`` of boxes / spheres / capsules / cylinders, or a list of up to 8 of them) into the hand:
        -> an ``Attachment`` (numbotics_amd.physics) of ``obj`` riding on ``link`` (a Link of this chain or its name).  ``pose``
        (4, 4): the grasp, the object's pose in the link frame (for a list: the first object's); default: the object where it
        stands now, relative to the link at ``arm.configuration``.  ``touch_links``: links (or names) the object may touch, e.g.
        the fingers.  The held shapes are paired with every world shape of ``scene_model()`` that is not the object's own and with
        every robot shape whose link is neither ``link``, nor shares its moving frame, nor is a touch link; the attachment is
        resolved again whenever the scene changes.  Check it with ``in_collision_with_attached`` or ``ConnectorParams(attached=...)``:
        ``in_collision`` does NOT see the held object, and still sees the object's world copy where it is one of this arm's
        obstacles -- park it or ``remove_collision_pair`` it.  ``meshes=True``: a ``Mesh`` may be held too, as its convex hulls -- one,
        or one per object of its file with ``convex_decomposition=True``, by the routine link meshes go through; the hulls count
        against the 8 shapes.  Such an attachment does not see scans by default: every ``cloud`` argument of the attached calls
        refuses it.  ``mesh_scans=True`` (with ``meshes=True``) opts in: the hulls are then served against point clouds by every
        attached call that takes a ``cloud`` and by both connectors' ``attached_sees_cloud``."""
        from numbotics_amd.physics import Attachment
        from .model import chain_link_poses
        link = self._resolve(link)
        if not self._in_chain(link):
            raise ValueError(f"Link {getattr(link, '_name', link)} not found in chain")
        objs = list(obj) if isinstance(obj, (list, tuple)) else [obj]
        if pose is None:
            if not objs or not isinstance(objs[0], PhysicsObject):
                raise ValueError("the held object must be a PhysicsObject or a list of them")
            pose = np.linalg.inv(chain_link_poses(self._chain)[link._name]) @ np.asarray(objs[0].pose, dtype=np.float64)
        att = Attachment(link, objs, pose, touch_links, meshes=meshes, mesh_scans=mesh_scans)
        att.spec(self)                                          # argument errors now, not at the first query
        return att

    def in_collision_with_attached(self, q, att, threshold: float = 0.0, pose=None, cloud=None):
        """Is the held object of ``att`` (``attach`` / ``World.add_constraint``) closer than ``threshold`` to a world shape or a
        link it is paired with?  ``(dof,)`` -> bool, ``(..., dof)`` -> bool array / tensor, like ``in_collision_with_cloud``.  This
        is the held object's verdict ONLY: full validity is ``arm.in_collision(q) | arm.in_collision_with_attached(q, att)``, and
        ``in_collision`` still sees the object's world copy where that is an obstacle of this arm.  ``pose``: another grasp for
        this call, (4, 4), or one per configuration (B, 4, 4) -- NumPy or a float64 CUDA tensor.  ``cloud`` (a ``PointCloud``):
        the held object's verdict against the scan is ORed in (``DeviceModel.held_cloud_validity``); without it the held object
        does not see a scan."""
        if q.shape[-1] != self.dof:
            raise ValueError(f"q must have {self.dof} elements")
        dev, held = att._device(self)
        if cloud is not None:
            dev._held_scanless(held)                              # (a held mesh: refused before anything runs)
        rows = q.reshape(-1, self.dof)
        mask = dev.held_validity(held, rows, threshold, pose=pose)
        if cloud is not None:
            mask = mask | dev.held_cloud_validity(held, cloud, rows, threshold, pose=pose)
        if q.ndim == 1:
            return bool(mask[0])
        return mask.reshape(tuple(q.shape[:-1]))

    def attached_cloud_clearance(self, q, att, cloud, d_max: float, pose=None):
        """How close is the held object of ``att`` to ``cloud``?  -> (distance, held shape index, point index): the smallest signed
        distance below ``d_max`` with the held shape and the point (its index in the cloud's last update) that attain it, or
        (inf, -1, -1) where nothing is nearer than ``d_max``; NaN, -1, -1 for a row or grasp that is not finite or while the
        cloud's status is set.  ``(dof,)`` -> (float, int, int); ``(B, dof)`` -> arrays / tensors (B,).  ``pose``: as
        ``in_collision_with_attached``."""
        if q.shape[-1] != self.dof:
            raise ValueError(f"q must have {self.dof} elements")
        dev, held = att._device(self)
        d, sh, pt = dev.held_cloud_clearance(held, cloud, q.reshape(-1, self.dof), d_max, pose=pose)
        if q.ndim == 1:
            return float(d[0]), int(sh[0]), int(pt[0])
        return d, sh, pt

    def attached_clearance(self, q, att, pose=None):
        """How close is the held object of ``att`` to what it is paired with?  -> (distance, item): the smallest signed distance
        over the attachment's items and the item that attains it (the smallest index on a tie; ``att.items(arm)`` names them), or
        (inf, -1) where the attachment has no item.  ``(dof,)`` -> (float, int); ``(B, dof)`` -> arrays / tensors (B,).  A row
        that is not finite gives NaN and -1.  ``pose``: as ``in_collision_with_attached``."""
        if q.shape[-1] != self.dof:
            raise ValueError(f"q must have {self.dof} elements")
        dev, held = att._device(self)
        d = dev.held_distances(held, q.reshape(-1, self.dof), pose=pose)
        if isinstance(d, np.ndarray):
            B = d.shape[0]
            if d.shape[1] == 0:
                dist, item = np.full((B,), np.inf), np.full((B,), -1, dtype=np.int64)
            else:
                bad = np.isnan(d).any(axis=1)
                item = np.where(bad, -1, np.argmin(np.where(np.isnan(d), np.inf, d), axis=1))
                dist = np.where(bad, np.nan, d[np.arange(B), np.maximum(item, 0)])
        else:
            import torch
            B = d.shape[0]
            if d.shape[1] == 0:
                dist = torch.full((B,), float("inf"), dtype=torch.float64, device=d.device)
                item = torch.full((B,), -1, dtype=torch.int64, device=d.device)
            else:
                bad = torch.isnan(d).any(dim=1)
                dmin = d.min(dim=1, keepdim=True).values
                k = torch.arange(d.shape[1], device=d.device).expand_as(d)
                first = torch.where(d == dmin, k, d.shape[1]).min(dim=1).values        # the smallest index that attains the minimum
                item = torch.where(bad, -1, first)
                dist = torch.where(bad, float("nan"), dmin[:, 0])
        if q.ndim == 1:
            return float(dist[0]), int(item[0])
        return dist, item

    # ---- records of the held object's items (additive): where it touches, along which normal, and the gradient of the distance ---
    def _attached(self, q, att):
        """The argument rules of the attached record calls, before anything touches the device -> (DeviceModel, DeviceHeld)."""
        from numbotics_amd.physics import Attachment
        if not isinstance(att, Attachment):
            raise ValueError("att must be an Attachment (Arm.attach / World.add_constraint)")
        self._check_q(q)
        return att._device(self)

    def attached_proximity_jacobians(self, q, att, pose=None, per_item=False):
        """``attached_clearance`` with the contact and the gradient, as ``closest_proximity_jacobians`` has it for the arm's own
        pairs: ``(..., dof)`` (flattened to B rows) -> dist ``(B,)``, item ``(B,)`` int32 (the first minimum; ``att.items(arm)``
        names them), witness ``(B, 9)``, rows ``(B, dof)``.  For a (held shape, link) item the subject is the LINK and the target
        the held object, for a (held shape, obstacle) item the subject is the held object: witness = point on the subject, point on
        the target, unit normal from the target to the subject; rows = n . Jv_subject - n . Jv_target, the gradient of the distance.
        A row that is not finite gives NaN, -1, NaN, NaN; no items: inf, -1, NaN, rows of zeros.  ``per_item=True``: every item,
        dist ``(B, K)``, witness ``(B, K, 9)``, rows ``(B, K, dof)`` (``DeviceModel.held_records``).  ``pose``: as
        ``in_collision_with_attached``.  The closest item and its record are found on the device, with no host round trip."""
        dev, held = self._attached(q, att)
        rows = q.reshape(-1, self.dof)
        if per_item:
            return dev.held_records(held, rows, pose=pose)
        return dev.held_closest_records(held, rows, pose=pose)

    def attached_closest_to(self, q, att, pose=None):
        """``closest_to`` for the held object of ``att``: the ``Proximity`` of its closest item -- subject = the link and target =
        the held object (``att.objects[0]``) for a (held shape, link) item, subject = the held object and target = the obstacle
        for a (held shape, obstacle) item -- or None for a ``q`` that is not finite or an attachment without items."""
        if tuple(q.shape) != (self.dof,):
            raise ValueError(f"q must be a 1D array with {self.dof} elements")
        dev, held = self._attached(q, att)
        qn = q.detach().cpu().numpy() if _is_tensor(q) else np.asarray(q, dtype=np.float64)
        d, item, w, _ = dev.held_closest_records(held, qn.reshape(1, -1), pose=pose)
        if item[0] < 0:
            return None
        sm = self.scene_model()
        _, kind, idx = (int(v) for v in held.items()[item[0]])
        if kind == 0:
            subj, targ = sm.links[sm.rshape_link[idx]], att.objects[0]
        else:
            subj, targ = att.objects[0], sm.objects[sm.wshape_obj[idx]]
        return Proximity(subject=subj, target=targ, position_on_subject=w[0, 0:3].copy(), position_on_target=w[0, 3:6].copy(),
                         normal_target_to_subject=w[0, 6:9].copy(), distance=float(d[0]))

    def attached_cloud_proximity_jacobians(self, q, att, cloud, d_max: float, pose=None, per_shape: bool = False):
        """``attached_cloud_clearance`` with the contact and the gradient, as ``cloud_proximity_jacobians`` has it for the links:
        (distance, held shape index, point index, witness, rows) per configuration of ``q`` (``(dof,)`` or ``(..., dof)``,
        flattened to B rows) -- witness ``(B, 9)`` = point on the held shape, point on the cloud point's sphere, unit normal from
        the point to the shape; rows ``(B, dof)`` = n . Jv_held(point on the shape).  Nothing nearer than ``d_max``: inf, -1, -1,
        NaN, a row of zeros (a hinge cost's gradient); a row or grasp that is not finite, or a set cloud status: NaN, -1, -1, NaN,
        NaN.  ``per_shape=True``: one record per (configuration, held shape), ``(B, H)`` ... ``(B, H, dof)``."""
        dev, held = self._attached(q, att)
        return dev.held_cloud_records(held, cloud, q.reshape(-1, self.dof), d_max, pose=pose, per_shape=per_shape)

    def attached_cloud_closest_to(self, q, att, cloud, d_max: float, pose=None):
        """``cloud_closest_to`` for the held object of ``att``: the ``Proximity`` of the closest (held shape, point) when it is
        nearer than ``d_max`` -- subject = the held object (``att.objects[0]``), target = ``cloud`` -- else None (also for a
        non-finite ``q``)."""
        if tuple(q.shape) != (self.dof,):
            raise ValueError(f"q must be a 1D array with {self.dof} elements")
        dev, held = self._attached(q, att)
        qn = q.detach().cpu().numpy() if _is_tensor(q) else np.asarray(q, dtype=np.float64)
        d, sh, _, w, _ = dev.held_cloud_records(held, cloud, qn.reshape(1, -1), d_max, pose=pose, jacobian=False)
        if sh[0] < 0:
            return None
        return Proximity(subject=att.objects[0], target=cloud, position_on_subject=w[0, 0:3].copy(),
                         position_on_target=w[0, 3:6].copy(), normal_target_to_subject=w[0, 6:9].copy(), distance=float(d[0]))

    def cloud_self_filter(self, points, q, radius: float, padding: float = 0.0, keep=None, links=None, ignore_links=()):
        """Which of a depth frame's ``points`` (N, 3) are NOT the arm's own image at the configuration ``q`` the frame was taken at:
        ``keep[i]`` goes to 0 iff point i, a sphere of ``radius``, is closer than ``padding`` to a link shape -- the verdict
        ``in_collision_with_cloud(q, cloud, padding)`` would give for that point alone, so a cloud updated with
        ``update(points, keep=keep)`` reads free at ``q``, exactly.  ``links``: only these links (objects or names; default: all);
        ``ignore_links``: links left out of the filter, whose image stays in the cloud.  ``keep``, the return value and the array
        kinds: as ``DeviceModel.cloud_self_filter``."""
        sm, dev = self._scene_device()
        shapes = self._cloud_shapes(sm, ignore_links)
        if links is not None:
            names = {getattr(l, "_name", l) for l in links}
            known = {l._name for l in sm.links}
            for n in names:
                if n not in known:
                    raise ValueError(f"Link {n} not found in chain")
            shapes = [s for s in (range(sm.n_rshapes) if shapes is None else shapes) if sm.links[sm.rshape_link[s]]._name in names]
        q = q.reshape(-1) if hasattr(q, "reshape") else np.asarray(q, dtype=np.float64).reshape(-1)
        if q.shape[0] != self.dof:
            raise ValueError(f"q must have {self.dof} elements")
        return dev.cloud_self_filter(points, q, radius, padding, keep=keep, shapes=shapes)

    def depth_images(self, q, camera_pose, width: int, height: int, fov: float = 60.0, intrinsics=None, near: float = 0.01,
                     far: float = 1000.0, frame: str = "numbotics", links=None, ignore_links=(), world: bool = True, labels: bool = False,
                     out=None):
        """Depth frames of the arm at ``q`` among its world's obstacles, ray-cast on the device (``DeviceModel.render_depth``): what
        a depth camera at ``camera_pose`` sees of the shapes ``in_collision`` checks, in the shape mode of this arm
        (``bullet_margins``).  ``q``: ``(dof,)`` or ``(B, dof)``; ``camera_pose``: one (4, 4) pose or ``(B, 4, 4)``; one of either
        serves the other's batch.  ``frame="numbotics"`` (the default, ``World.depth_image``'s camera: looking along x, z up) or
        ``"optical"``.  ``fov`` is the vertical field of view in degrees (``intrinsics_from_fov``) unless ``intrinsics`` -- (fx, fy,
        cx, cy) or a 3 x 3 matrix -- is given.  ``links`` / ``ignore_links``: draw only / all but these links; ``world=False``: the
        arm alone.  -> the metric depth along the view axis, float32 ``(height, width)`` for one ``q`` and one pose, else ``(B,
        height, width)``; 0 where nothing is seen within [near, far] -- a hole to ``backproject``.  ``labels=True``: (depth, label)
        with the shape behind each pixel (``SceneModel`` order; ``n_rshapes + w`` for world shape w, -1 nothing, -2 undecided).
        NumPy ``q`` gives NumPy, a CUDA ``q`` CUDA tensors, which ``PointCloud.update_from_depth`` / ``integrate_depth`` take as
        they are.  ``out``: as ``DeviceModel.render_depth``."""
        from numbotics_amd.physics.pointcloud import intrinsics_from_fov
        sm, dev = self._scene_device()
        shapes = self._cloud_shapes(sm, ignore_links)
        if links is not None:
            names = {getattr(l, "_name", l) for l in links}
            known = {l._name for l in sm.links}
            for n in names:
                if n not in known:
                    raise ValueError(f"Link {n} not found in chain")
            shapes = [s for s in (range(sm.n_rshapes) if shapes is None else shapes) if sm.links[sm.rshape_link[s]]._name in names]
        is_np = isinstance(q, np.ndarray) or not hasattr(q, "is_cuda")
        if is_np:
            q = np.asarray(q, dtype=np.float64)
        if q.shape[-1] != self.dof:
            raise ValueError(f"q must have {self.dof} elements")
        if not hasattr(camera_pose, "ndim"):
            camera_pose = np.asarray(camera_pose, dtype=np.float64)
        one = q.ndim == 1 and camera_pose.ndim == 2
        k = intrinsics if intrinsics is not None else intrinsics_from_fov(width, height, fov)
        res = dev.render_depth(q.reshape(-1, self.dof), camera_pose, k, height, width, near=near, far=far, shapes=shapes, world=world,
                               out=out, labels=labels, frame=frame)
        parts = res if labels else (res,)
        if one:
            parts = tuple(p.reshape(int(height), int(width)) for p in parts)
        if is_np:
            parts = tuple(p.cpu().numpy() for p in parts)
        return parts if labels else parts[0]

    def cloud_clearance(self, q, cloud, d_max: float, ignore_links=()):
        """(distance, link name, point index) per configuration: the smallest signed distance between a link shape and a point of
        ``cloud`` when it is below ``d_max`` (else inf, None, -1; NaN, None, -1 for a non-finite configuration).  ``q`` is
        ``(dof,)`` or ``(B, dof)``; distances and point indices come back as arrays (or tensors, for a tensor ``q``), the link
        names as an object array."""
        if q.shape[-1] != self.dof:
            raise ValueError(f"q must have {self.dof} elements")
        sm, dev = self._scene_device()
        d, sh, pt = dev.cloud_clearance(cloud, q.reshape(-1, self.dof), d_max, shapes=self._cloud_shapes(sm, ignore_links))
        shn = sh.cpu().numpy() if _is_tensor(sh) else sh
        names = np.array([sm.links[sm.rshape_link[s]]._name if s >= 0 else None for s in shn], dtype=object)
        return d, names, pt

    def _link_names(self, sm, sh):
        shn = sh.cpu().numpy() if _is_tensor(sh) else sh
        flat = [sm.links[sm.rshape_link[s]]._name if s >= 0 else None for s in shn.reshape(-1)]
        out = np.empty((len(flat),), dtype=object)
        out[:] = flat
        return out.reshape(shn.shape)

    def cloud_proximity_jacobians(self, q, cloud, d_max: float, ignore_links=(), per_shape: bool = False):
        """``cloud_clearance`` with the contact and the gradient: (distance, link names, point index, witness, rows) per
        configuration of ``q`` (``(dof,)`` or ``(..., dof)``, flattened to B rows) -- witness ``(B, 9)`` = point on the link's
        shape, point on the cloud point's sphere, unit normal from the point to the shape; rows ``(B, dof)`` = n . Jv_link(point on
        the shape), the gradient of the distance.  Nothing nearer than ``d_max``: inf, None, -1, NaN, a row of zeros (a hinge
        cost's gradient).  ``per_shape=True``: one record per (configuration, link shape left after ``ignore_links``), ``(B, S)``,
        ``(B, S)``, ``(B, S)``, ``(B, S, 9)``, ``(B, S, dof)``, and a sixth value: the link names of the S columns."""
        sm = self.scene_model()
        self._check_q(q)
        shapes = self._cloud_shapes(sm, ignore_links)
        _, dev = self._scene_device()
        d, sh, pt, w, j = dev.cloud_records(cloud, q.reshape(-1, self.dof), d_max, shapes=shapes, per_shape=per_shape)
        if not per_shape:
            return d, self._link_names(sm, sh), pt, w, j
        cols = range(sm.n_rshapes) if shapes is None else shapes
        return d, self._link_names(sm, sh), pt, w, j, np.array([sm.links[sm.rshape_link[s]]._name for s in cols], dtype=object)

    def cloud_closest_to(self, q, cloud, d_max: float, ignore_links=()):
        """``closest_to`` for a cloud: the ``Proximity`` of the closest (link shape, point) when it is nearer than ``d_max`` --
        subject = the link, target = ``cloud`` -- else None (also for a non-finite ``q``)."""
        if tuple(q.shape) != (self.dof,):
            raise ValueError(f"q must be a 1D array with {self.dof} elements")
        sm = self.scene_model()
        shapes = self._cloud_shapes(sm, ignore_links)
        _, dev = self._scene_device()
        qn = q.detach().cpu().numpy() if _is_tensor(q) else np.asarray(q, dtype=np.float64)
        d, sh, _, w, _ = dev.cloud_records(cloud, qn.reshape(1, -1), d_max, shapes=shapes, jacobian=False)
        if sh[0] < 0:
            return None
        return Proximity(subject=sm.links[sm.rshape_link[sh[0]]], target=cloud, position_on_subject=w[0, 0:3].copy(),
                         position_on_target=w[0, 3:6].copy(), normal_target_to_subject=w[0, 6:9].copy(), distance=float(d[0]))

    def pair_distances(self, q):
        """(B, P) signed distances of every allowed primitive pair (additive, batched ``collisions``)."""
        sm, dev = self._scene_device()
        return dev.pair_distances(q.reshape(-1, self.dof))

    def closest_distance(self, q):
        """(B,) min signed distance and (B,) pair index (additive, batched ``closest_to``)."""
        sm, dev = self._scene_device()
        return dev.closest(q.reshape(-1, self.dof))

    def _pair_selection(self, sm, obj, link):
        """Indices (into the scene's primitive pair list) of the proximities ``distance_to(q, obj, link)`` returns."""
        pairs = self.collision_pairs()
        sel = []
        for p in range(sm.n_pairs):
            subj, targ = sm.pair_members(p)
            if not (targ == obj or (isinstance(obj, Chain) and self._in_chain(targ) and obj == self._chain)):
                continue
            if link is None:
                if self._has(pairs, subj, targ):
                    sel.append(p)
            elif subj == link:
                sel.append(p)
        return sel

    def distance_to(self, q, obj, link=None):
        """As upstream: the Proximity records of ``collisions(q)`` that involve ``obj`` (and ``link``) -- computed for those
        pairs only (the subset path, bit-identical to the all-pairs records)."""
        if link is not None and not self._has(self.collision_pairs(), link, obj):
            raise ValueError(f"Collision pair ({link.name}, {obj.name}) not valid")
        if tuple(q.shape) != (self.dof,):
            raise ValueError(f"q must be a 1D array with {self.dof} elements")
        sm, dev = self._scene_device()
        sel = self._pair_selection(sm, obj, link)
        if not sel:
            return []
        qn = q.detach().cpu().numpy() if _is_tensor(q) else np.asarray(q, dtype=np.float64)
        dist, wit, _ = self._subset_records(dev, qn.reshape(1, -1), np.asarray(sel, dtype=np.int64), jacobian=False)
        return self._proximities(sm, sel, dist[0], wit[0])

    def proximity_jacobians(self, q):
        """Batched ``collisions`` + ``jacobian_proximity`` over every allowed primitive pair (additive):
        ``(..., dof)`` -> signed distances ``(B, P)``, witnesses ``(B, P, 9)`` (point on subject, point on target,
        normal target->subject) and rows ``(B, P, dof)`` with row = n . Jv_subject(p_s) - n . Jv_target(p_t)
        (arm.py:620-632), one launch."""
        sm, dev = self._scene_device()
        return dev.proximity_jacobian(q.reshape(-1, self.dof))

    # ---- records of chosen pairs (additive) ----------------------------------------------------------------
    # The same records and rows as proximity_jacobians, bit for bit, computed for the (configuration, pair) items asked for
    # only (nbk_pair_records_items).  Arguments are checked against scene_model() before anything touches the device.
    def _check_q(self, q):
        if q.ndim < 1 or q.shape[-1] != self.dof:
            raise ValueError(f"q must have {self.dof} elements in its last dimension")

    @staticmethod
    def _check_pair_values(a, n_pairs, what):
        if a.size and (int(a.min()) < 0 or int(a.max()) >= n_pairs):
            raise ValueError(f"{what}: pair index out of range [0, {n_pairs})")

    def _pair_indices(self, sm, pairs):
        a = pairs.detach().cpu().numpy() if _is_tensor(pairs) else np.asarray(pairs)
        if a.ndim != 1:
            raise ValueError("pairs must be a 1-D sequence of pair indices")
        if a.size and (a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer)):
            raise ValueError("pairs must hold integer pair indices")
        self._check_pair_values(a, sm.n_pairs, "pairs")
        return a.astype(np.int64)

    def _subset_records(self, dev, q, sel, witness=True, jacobian=True):
        """Records of the pairs ``sel`` for every row of q: (B, S), (B, S, 9), (B, S, dof).  Items go pair-major, so that each
        wave of 64 items holds one pair."""
        q2 = q.reshape(-1, self.dof)
        B, S = int(q2.shape[0]), int(sel.size)
        if _is_tensor(q2):
            import torch
            dv = q2.device if q2.is_cuda else torch.device("cuda")
            b = torch.arange(B, dtype=torch.int32, device=dv).repeat(S)
            p = torch.from_numpy(sel.astype(np.int32)).to(dv).repeat_interleave(B)
            items = torch.stack((b, p), dim=1)
        else:
            items = np.stack((np.tile(np.arange(B, dtype=np.int32), S), np.repeat(sel.astype(np.int32), B)), axis=1)
        d, w, j = dev.pair_records(q2, items, witness=witness, jacobian=jacobian)

        def batch_major(x, tail):
            if x is None:
                return None
            x = x.reshape((S, B) + tail)
            perm = (1, 0) + tuple(range(2, 2 + len(tail)))
            return x.permute(*perm).contiguous() if _is_tensor(x) else np.ascontiguousarray(x.transpose(perm))
        return batch_major(d, ()), batch_major(w, (9,)), batch_major(j, (self.dof,))

    def pair_proximity_jacobians(self, q, pairs):
        """``proximity_jacobians(q)`` restricted to the columns ``pairs`` (1-D user pair indices, repeats and any order allowed):
        ``(..., dof)`` -> ``(B, S)``, ``(B, S, 9)``, ``(B, S, dof)``, bit-identical to ``proximity_jacobians(q)[:, pairs]``."""
        sm = self.scene_model()
        sel = self._pair_indices(sm, pairs)
        self._check_q(q)
        _, dev = self._scene_device()
        return self._subset_records(dev, q, sel)

    def item_proximity_jacobians(self, q, pair):
        """One pair per configuration: ``pair`` (B,) user pair indices (NumPy or a CUDA tensor) -> ``(B,)``, ``(B, 9)``,
        ``(B, dof)``, the records of ``proximity_jacobians(q)`` at [b, pair[b]].  (A CUDA tensor's range check reads its min and
        max back.)"""
        sm = self.scene_model()
        self._check_q(q)
        B = int(np.prod(q.shape[:-1])) if q.ndim > 1 else 1
        if _is_tensor(pair):
            import torch
            if pair.ndim != 1 or pair.shape[0] != B:
                raise ValueError(f"pair must have shape ({B},)")
            if pair.dtype == torch.bool or pair.is_floating_point() or pair.is_complex():
                raise ValueError("pair must hold integer pair indices")
            if B:
                self._check_pair_values(torch.stack((pair.min(), pair.max())).cpu().numpy(), sm.n_pairs, "pair")
            dv = pair.device if pair.is_cuda else torch.device("cuda")
            items = torch.stack((torch.arange(B, dtype=torch.int32, device=dv), pair.to(device=dv, dtype=torch.int32)), dim=1)
        else:
            a = np.asarray(pair)
            if a.shape != (B,):
                raise ValueError(f"pair must have shape ({B},)")
            if a.size and (a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer)):
                raise ValueError("pair must hold integer pair indices")
            self._check_pair_values(a, sm.n_pairs, "pair")
            items = np.stack((np.arange(B, dtype=np.int32), a.astype(np.int32)), axis=1)
        _, dev = self._scene_device()
        return dev.pair_records(q.reshape(-1, self.dof), items)

    def closest_proximity_jacobians(self, q):
        """Batched ``closest_to`` + ``jacobian_proximity`` of the closest pair (the greedy counter-example search,
        safe_sets.py:137-152): ``(..., dof)`` -> dist ``(B,)``, pair ``(B,)`` int32 (first minimum), witness ``(B, 9)``,
        rows ``(B, dof)``.  The closest-pair kernel and the item kernel run back to back on the device."""
        sm = self.scene_model()
        self._check_q(q)
        if sm.n_pairs == 0:
            raise ValueError("min() arg is an empty sequence")
        _, dev = self._scene_device()
        return dev.closest_records(q.reshape(-1, self.dof))

    def jacobian_proximity(self, q, obj, link=None):
        """As upstream (arm.py:620-632): one row per proximity of ``distance_to(q, obj, link)``, a 1-D row when
        there is exactly one."""
        if tuple(q.shape) != (self.dof,):
            raise ValueError(f"q must be a 1D array with {self.dof} elements")
        if link is not None and not self._has(self.collision_pairs(), link, obj):
            raise ValueError(f"Collision pair ({link.name}, {obj.name}) not valid")
        sm, dev = self._scene_device()
        sel = self._pair_selection(sm, obj, link)
        qn = q.detach().cpu().numpy() if _is_tensor(q) else np.asarray(q, dtype=np.float64)
        if not sel:
            return np.zeros((0, self.dof))
        _, _, rows = self._subset_records(dev, qn.reshape(1, -1), np.asarray(sel, dtype=np.int64), witness=False)
        J = np.ascontiguousarray(rows[0])
        if J.shape[0] == 1:
            return J[0]
        return J
