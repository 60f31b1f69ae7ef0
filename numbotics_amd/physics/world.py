"""World registry (reference: numbotics/physics/world.py:24-64,213-259).

Only the object registries the hot path reads (``_static_objects`` / ``_dynamic_objects``, iterated at
robots/arm.py:228,564) are kept.  There is no PyBullet client, stepping, visualiser or
constraint store: simulation is out of scope.  ``World.pool`` (world.py:98-156)
exists upstream to clone PyBullet worlds for CPU threads; the device path batches instead, so it is
not reproduced.
"""
import itertools
import weakref
from typing import Any

WORLD_INSTANCES: dict = {}
SELECTED_WORLD = None


def get_world(name=None):
    global SELECTED_WORLD
    if name is None:
        name = SELECTED_WORLD
    if name is None and len(WORLD_INSTANCES) == 0:
        name = 'world_0'
    if name is None:
        raise ValueError('There should always be a selected World instance if a World exists')
    if name not in WORLD_INSTANCES:
        World(name=name)
    SELECTED_WORLD = name
    return WORLD_INSTANCES[name]


class World:

    def __init__(self, name=None, visualize: bool = False):
        global SELECTED_WORLD
        if visualize:
            raise NotImplementedError("visualisation is out of scope for the MI355X hot path")
        if name in WORLD_INSTANCES:
            raise ValueError(f'World with name {name} already exists')
        self._name = f'world_{len(WORLD_INSTANCES)}' if name is None else name
        WORLD_INSTANCES[self._name] = self
        SELECTED_WORLD = self._name
        # weak, like upstream: a body that goes out of scope leaves the world.
        self._static_objects = weakref.WeakValueDictionary()
        self._dynamic_objects = weakref.WeakValueDictionary()
        self._entity_map = weakref.WeakValueDictionary()
        self._ids = itertools.count()
        self._vis = None
        self._revision = 0          # bumped whenever the scene changes; device scenes key on it
        self._attachments = []      # held objects recorded by add_constraint (physics/attachment.py)
        self.gravity = None

    @property
    def name(self):
        return self._name

    def _next_id(self) -> int:
        return next(self._ids)

    def _touch(self):
        self._revision += 1

    def register(self, body):
        from .object import PhysicsObject
        from .chain import Chain
        if not isinstance(body, (PhysicsObject, Chain)):
            raise ValueError(f"Unknown body type: {type(body)}")
        if body._static:
            self._static_objects[body.name] = body
        else:
            self._dynamic_objects[body.name] = body
        self._entity_map[body._pyb_id] = body
        self._touch()

    def unregister(self, body):
        for reg in (self._static_objects, self._dynamic_objects):
            if body.name in reg:
                del reg[body.name]
        self._entity_map.pop(body._pyb_id, None)
        self._touch()

    def objects(self):
        return list(self._static_objects.values()) + list(self._dynamic_objects.values())

    def get_object(self, name: str, default: Any = None):
        from .chain import Chain
        if name in self._static_objects:
            return self._static_objects[name]
        if name in self._dynamic_objects:
            return self._dynamic_objects[name]
        for obj in list(self._dynamic_objects.values()) + list(self._static_objects.values()):
            if isinstance(obj, Chain):
                for link in obj._links:
                    if link.name == name:
                        return link
        return default

    def add_constraint(self, body1, body2, constraint):
        """The reference's signature (numbotics/physics/world.py:315-360).  A FIXED ``Joint`` between a chain ``Link`` and a
        ``PhysicsObject``, in either order, records an ``Attachment`` (physics/attachment.py): the object rides on the link at the
        grasp the joint's ``offset`` / ``parent_pose`` / ``child_pose`` stand for (``constraint_grasp``) and is checked with
        ``Arm.in_collision_with_attached`` / ``ConnectorParams(attached=...)``; it is returned, and listed by ``attachments()``.
        Upstream's constraint is a Bullet dynamics constraint, this one a kinematic attachment for collision checks; every other
        combination raises ``NotImplementedError``, as upstream does for the types it does not support."""
        from .attachment import Attachment, constraint_grasp
        from .chain import Link
        from .constraint import Constraint
        from .object import PhysicsObject
        if getattr(constraint, "type", None) != Constraint.FIXED:
            raise NotImplementedError(f"Only fixed constraints between a link and an object are supported, got {getattr(constraint, 'type', constraint)}")
        if isinstance(body1, Link) and isinstance(body2, PhysicsObject):
            link, obj, link_first = body1, body2, True
        elif isinstance(body1, PhysicsObject) and isinstance(body2, Link):
            link, obj, link_first = body2, body1, False
        else:
            raise NotImplementedError("Only a chain Link and a PhysicsObject can be constrained, got "
                                      f"{type(body1).__name__} and {type(body2).__name__}")
        att = Attachment(link, obj, constraint_grasp(constraint, link_first))
        self._attachments.append(att)
        return att

    def attachments(self):
        """The attachments recorded by ``add_constraint``, oldest first."""
        return list(self._attachments)

    def step(self):
        """No dynamics here; kept so reference scripts that call ``world.step()`` still run."""
        return None

    def static_scene(self, bullet_margins: bool = True):
        """Every registered body as it stands -- chains at their ``configuration`` -- as the world shapes of a zero-joint
        ``SceneModel`` without robot shapes and pairs (the route of physics/proximity.py): what ``depth_image`` draws.  World shape
        w belongs to ``wshape_obj[w]`` of ``objects()``.  Needs no GPU."""
        from numbotics_amd.robots.model import HullTable, _shape_records
        from .proximity import _static_shapes
        hulls = HullTable()
        ws, owner = [], []
        for k, body in enumerate(self.objects()):
            for _, cs, pose in _static_shapes(body):
                for t, T, p in _shape_records(cs, pose, hulls, bullet_margins):
                    ws.append((t, T, p))
                    owner.append(k)
        return static_scene_model(ws, hulls, owner)

    def depth_image(self, width: int, height: int, camera_pose, near: float = 0.01, far: float = 1000, fov: float = 60,
                    bullet_margins: bool = True):
        """The depth frame a camera at ``camera_pose`` sees of every registered body (reference: numbotics/physics/world.py:363-398,
        Bullet's ``getCameraImage`` linearised) -> ``(height, width, 1)`` float64, the metric depth along the view axis; ``far``
        where nothing is seen, the value Bullet's cleared depth buffer linearises to.  The camera stands at ``camera_pose[:3, 3]``
        and looks along the pose's x axis with z up (the reference's comment); ``fov`` is the vertical field of view
        in degrees, the aspect ``width / height`` (``intrinsics_from_fov``).  Ray-cast on the device on the shapes and distances the
        collision checks use (``DeviceModel.render_depth``), boxes, cylinders and hulls rounded by Bullet's margins unless
        ``bullet_margins=False`` (additive).  Parity with Bullet's rasteriser is unpinned.  A GPU is required."""
        import numpy as np
        from numbotics_amd.engine import DeviceModel
        from .pointcloud import intrinsics_from_fov
        # (a descriptor per call: a few small uploads against a frame's rays, and no cache to keep right)
        dev = DeviceModel(self.static_scene(bullet_margins))
        depth, label = dev.render_depth(np.zeros((1, 1)), np.asarray(camera_pose, dtype=np.float64), intrinsics_from_fov(width, height, fov),
                                        height, width, near=near, far=far, labels=True, frame="numbotics")
        d = depth.cpu().numpy().astype(np.float64).reshape(int(height), int(width))
        d[label.cpu().numpy().reshape(d.shape) < 0] = float(far)
        return d.reshape(int(height), int(width), 1)


def static_scene_model(records, hulls=None, owners=None):
    """World shape records [(type, 4x4 world pose, params[4])] (robots/model.py: ``_shape_records``) as a zero-joint ``SceneModel``
    without robot shapes and pairs: a scene that is drawn, never checked.  ``hulls``: the ``HullTable`` the records' hulls name."""
    import numpy as np
    from numbotics_amd.robots.model import KinematicModel, SceneModel, HullTable, _T34
    W = len(records)
    z = np.zeros
    kin = KinematicModel(n_q=1, joint_parent=z(0, dtype=np.int32), joint_type=z(0, dtype=np.int32), joint_qidx=z(0, dtype=np.int32),
                         joint_offset=z((0, 12)), joint_axis=z((0, 3)), joint_rot=z((0, 27)), joint_trans=z((0, 3)), joint_slide=z((0, 3)),
                         base_pose=_T34(np.eye(4)))
    hvb, hv, hfb, hp = (hulls if hulls is not None else HullTable()).arrays()
    return SceneModel(kin=kin, rshape_frame=z(0, dtype=np.int32), rshape_type=z(0, dtype=np.int32), rshape_local=z((0, 12)),
                      rshape_param=z((0, 4)), rshape_link=z(0, dtype=np.int32), wshape_type=np.array([r[0] for r in records], dtype=np.int32),
                      wshape_pose=np.array([_T34(r[1]) for r in records], dtype=np.float64).reshape(W, 12),
                      wshape_param=np.array([r[2] for r in records], dtype=np.float64).reshape(W, 4),
                      wshape_obj=np.asarray(owners if owners is not None else z(W), dtype=np.int32),
                      pair_a=z(0, dtype=np.int32), pair_b=z(0, dtype=np.int32),
                      hull_vert_begin=hvb, hull_verts=hv, hull_face_begin=hfb, hull_planes=hp)


def _reset_worlds():
    """Test helper: forget every world."""
    global SELECTED_WORLD
    WORLD_INSTANCES.clear()
    SELECTED_WORLD = None
