"""Held objects: a body (or several) attached to a link of a chain and carried through the scene -- what every pick-and-place query
has in the hand.  The reference's entry is ``World.add_constraint(body1, body2, Joint(FIXED))`` (numbotics/physics/world.py:315-360),
a Bullet dynamics constraint; here it is a kinematic attachment for collision checks ("Held objects").

An ``Attachment`` names the holding link, the held ``PhysicsObject``s, the grasp ``pose`` (the object's pose in the link frame; for a
list of objects the frame of the first) and the ``touch_links`` the object may touch.  ``spec(arm)`` resolves it against the arm's
``scene_model()`` into flat arrays (a ``HeldSpec``); the device object (``engine.DeviceHeld``) is made from those on first use and
again whenever the arm's scene cache is retired.

A held ``Mesh`` is opt-in (``meshes=True``): it is then held as its convex hulls, by the routine link meshes go through, and the spec
carries their hull tables (``engine.DeviceHeld(..., hulls=...)``, nbk_held_create_hulls).  Such an attachment is served against the
scene; against point clouds it is served only with ``mesh_scans=True`` as well (``engine.DeviceHeld(..., scans=True)``,
nbk_held_set_cloud_hulls) -- without that flag the held-versus-cloud calls refuse it ("Held hulls").

Geometry: the world pose of held shape h at q is ``F(q) . ((A . G) . L_h)`` -- F the moving frame of the link's joint, A the link's
constant pose in it (``kin.frames[link].local``), G the grasp, L_h the shape in the object's frame.

Pairs: every held shape with every world shape of the arm's scene except those of the held objects themselves, and with every robot
shape whose link is neither the holding link, nor shares its moving frame, nor is one of ``touch_links``.  This is the held object's
verdict ONLY: ``Arm.in_collision`` does not see the held object, and still sees its world copy where it is one of the arm's obstacles
-- the caller parks or unpairs that copy (``arm.remove_collision_pair``).
"""
from dataclasses import dataclass, field

import numpy as np

from numbotics_amd.utils import Shape

MAX_HELD_SHAPES = 8


@dataclass
class HeldSpec:
    """An ``Attachment`` resolved against one ``SceneModel``: what ``engine.DeviceHeld`` is made from."""
    frame: int                  # moving frame of the holding link (-1: the base)
    A: np.ndarray               # (4, 4) the link in that frame
    G: np.ndarray               # (4, 4) the grasp
    shape_local: np.ndarray     # (H, 4, 4) L_h
    shape_type: np.ndarray      # (H,) int32, robots.model SH_*
    shape_param: np.ndarray     # (H, 4)
    world_shapes: np.ndarray    # allowed world shapes of the scene, ascending
    robot_shapes: np.ndarray    # allowed robot shapes of the scene (SceneModel order), ascending
    # the hull tables of the held SH_HULL shapes (``HullTable.arrays()``; a hull shape names its hull in shape_param[h][0]); empty: none
    hull_vert_begin: np.ndarray = field(default_factory=lambda: np.zeros(1, dtype=np.int32))
    hull_verts: np.ndarray = field(default_factory=lambda: np.zeros((0, 3), dtype=np.float64))
    hull_face_begin: np.ndarray = field(default_factory=lambda: np.zeros(1, dtype=np.int32))
    hull_planes: np.ndarray = field(default_factory=lambda: np.zeros((0, 4), dtype=np.float64))

    @property
    def n_shapes(self):
        return int(self.shape_type.shape[0])

    @property
    def n_hulls(self):
        return int(np.asarray(self.hull_vert_begin).shape[0]) - 1

    @property
    def hulls(self):
        """(vert_begin, verts, face_begin, planes) for ``engine.DeviceHeld(hulls=...)``, or None without held hulls."""
        if self.n_hulls <= 0:
            return None
        return self.hull_vert_begin, self.hull_verts, self.hull_face_begin, self.hull_planes


def _pose44(pose, what="pose"):
    T = np.asarray(pose, dtype=np.float64)
    if T.shape != (4, 4) or not np.all(np.isfinite(T)):
        raise ValueError(f"{what} must be a finite (4, 4) pose")
    return T.copy()


class Attachment:

    def __init__(self, link, objects, pose, touch_links=(), meshes=False, mesh_scans=False):
        from .object import PhysicsObject
        from .chain import Link
        if not isinstance(link, Link):
            raise ValueError("an attachment needs a Link of a chain")
        objects = list(objects) if isinstance(objects, (list, tuple)) else [objects]
        if not objects or not all(isinstance(o, PhysicsObject) for o in objects):
            raise ValueError("the held object must be a PhysicsObject or a list of them")
        self.link = link
        self.objects = tuple(objects)
        self.pose = _pose44(pose)
        self.touch_links = tuple(getattr(l, "_name", l) for l in touch_links)
        self.meshes = bool(meshes)  # a held Mesh becomes convex hulls (one, or one per file object with convex_decomposition)
        if mesh_scans and not meshes:
            raise ValueError("mesh_scans=True needs meshes=True: it lets the convex hulls of a held mesh see point clouds")
        self.mesh_scans = bool(mesh_scans)  # the hulls of a held Mesh are served against point clouds too
        self._spec = None           # (arm id, scene key, HeldSpec)
        self._dev = None            # (DeviceModel, HeldSpec, DeviceHeld)

    @property
    def has_mesh(self):
        """A held object is a mesh (held as convex hulls): the held-versus-cloud calls refuse the attachment unless it was made
        with ``mesh_scans=True``."""
        return any(o._collision_shape.shape == Shape.MESH for o in self.objects)

    def shape_records(self, bullet_margins=True, hulls=None):
        """[(type, (4, 4) pose in the object's frame, params[4])] of the held shapes, by the routine link shapes go through
        (robots/model.py ``_shape_records``: the descriptor's shape mode decides the margins).  ``hulls``: the ``HullTable`` the
        hulls of held meshes are added to (``meshes=True`` attachments)."""
        from numbotics_amd.robots.model import HullTable, _shape_records
        first = self.objects[0].pose
        if hulls is None:
            hulls = HullTable()
        out = []
        for k, obj in enumerate(self.objects):
            cs = obj._collision_shape
            if cs.shape == Shape.EMPTY:
                continue
            if cs.shape == Shape.PLANE:
                raise ValueError("a held object cannot be a PLANE: boxes, spheres, capsules, cylinders and meshes only")
            if cs.shape == Shape.MESH and not self.meshes:
                raise ValueError("a held object cannot be a MESH unless the attachment opts in: pass meshes=True "
                                 "(it is then held as its convex hulls)")
            owner = np.eye(4) if k == 0 else np.linalg.inv(first) @ obj.pose
            out.extend(_shape_records(cs, owner, hulls, bullet_margins))
        if not out:
            raise ValueError("the held object has no collision shape")
        if len(out) > MAX_HELD_SHAPES:
            raise ValueError(f"a held object has at most {MAX_HELD_SHAPES} shapes, got {len(out)}")
        return out

    def spec(self, arm) -> HeldSpec:
        """This attachment against ``arm.scene_model()`` as it stands (cached until the arm's scene changes)."""
        if not arm._in_chain(self.link):
            raise ValueError(f"Link {self.link._name} not found in chain")
        sm = arm.scene_model()
        key = (id(arm), arm._scene_cache[0])
        if self._spec is not None and self._spec[0] == key:
            return self._spec[1]
        names = {l._name for l in sm.links}
        for n in self.touch_links:
            if n not in names:
                raise ValueError(f"Link {n} not found in chain")
        fr = sm.kin.frames[self.link._name]
        from numbotics_amd.robots.model import HullTable
        hulls = HullTable()
        recs = self.shape_records(arm._bullet_margins, hulls)
        vb, hv, fb, hp = hulls.arrays()
        held = {id(o) for o in self.objects}
        world = [w for w in range(sm.n_wshapes) if id(sm.objects[sm.wshape_obj[w]]) not in held]
        exempt = set(self.touch_links) | {self.link._name}
        robot = [s for s in range(sm.n_rshapes)
                 if int(sm.rshape_frame[s]) != fr.joint and sm.links[sm.rshape_link[s]]._name not in exempt]
        spec = HeldSpec(frame=int(fr.joint), A=np.array(fr.local, dtype=np.float64), G=self.pose.copy(),
                        shape_local=np.array([r[1] for r in recs], dtype=np.float64).reshape(-1, 4, 4),
                        shape_type=np.array([r[0] for r in recs], dtype=np.int32),
                        shape_param=np.array([r[2] for r in recs], dtype=np.float64).reshape(-1, 4),
                        world_shapes=np.array(world, dtype=np.int32), robot_shapes=np.array(robot, dtype=np.int32),
                        hull_vert_begin=vb, hull_verts=hv, hull_face_begin=fb, hull_planes=hp)
        self._spec = (key, spec)
        return spec

    def items(self, arm):
        """[(held shape, name)] of the attachment's items against ``arm.scene_model()``, in the order of the columns of
        ``DeviceModel.held_distances`` and of ``Arm.attached_clearance``'s item index: each held shape with the link (its name) of
        every allowed robot shape, robot shapes ascending, then with the object (its name, or its index among the scene's objects)
        of every allowed world shape, held shapes ascending.  Needs no GPU."""
        spec = self.spec(arm)
        sm = arm.scene_model()
        out = [(h, sm.links[sm.rshape_link[s]]._name) for s in spec.robot_shapes for h in range(spec.n_shapes)]
        for h in range(spec.n_shapes):
            for w in spec.world_shapes:
                o = int(sm.wshape_obj[w])
                out.append((h, getattr(sm.objects[o], "_name", None) or o))
        return out

    def _device(self, arm):
        """(DeviceModel, DeviceHeld) for the arm's current device scene."""
        from numbotics_amd.engine import DeviceHeld
        spec = self.spec(arm)
        _, dev = arm._scene_device()
        if self._dev is None or self._dev[0] is not dev or self._dev[1] is not spec:
            held = DeviceHeld(dev, spec.frame, spec.A, spec.G, spec.shape_type, spec.shape_local, spec.shape_param,
                              spec.world_shapes, spec.robot_shapes, hulls=spec.hulls, scans=self.mesh_scans)
            self._dev = (dev, spec, held)
        return dev, self._dev[2]


def constraint_grasp(constraint, link_first: bool) -> np.ndarray:
    """The grasp a FIXED ``Joint`` between a link and an object stands for.  The reference hands Bullet the two frames
    ``offset @ parent_pose`` (in body1) and ``offset @ child_pose`` (in body2), which the constraint keeps coincident:
    ``T_1 P = T_2 C``.  With the link first the object sits at ``P C^-1`` in the link frame, with the object first at ``C P^-1``."""
    eye = np.eye(4)
    off = np.asarray(constraint.offset, dtype=np.float64)
    P = off @ (eye if constraint.parent_pose is None else np.asarray(constraint.parent_pose, dtype=np.float64))
    Cp = off @ (eye if constraint.child_pose is None else np.asarray(constraint.child_pose, dtype=np.float64))
    return P @ np.linalg.inv(Cp) if link_first else Cp @ np.linalg.inv(P)
