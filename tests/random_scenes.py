"""Random mechanisms + obstacle sets for the fuzz tests (build-authored; nothing here comes from the reference)."""
import numpy as np


def random_hull_obj(rng, path, n_objects=1, scale=0.1):
    """A mesh file of ``n_objects`` random convex polytopes (one OBJ object each)."""
    from numbotics_amd.utils.mesh import write_obj, hull_faces
    parts = []
    for i in range(n_objects):
        n = int(rng.integers(6, 28))
        pts = rng.normal(size=(n, 3))
        pts = pts / np.linalg.norm(pts, axis=1, keepdims=True) * rng.uniform(0.5, 1.0, (n, 1)) * rng.uniform(0.3, 1.0, 3) * scale
        V, F = hull_faces(pts + rng.uniform(-scale, scale, 3) * (i > 0))
        parts.append((f"part{i}", V, F))
    return write_obj(path, parts)


def random_urdf(rng, n_links, path, max_back=3, meshes=False):
    """A random tree of n_links links: revolute / continuous / prismatic / fixed joints with random origins and
    axes, every link carrying 0-2 collision primitives (box / sphere / cylinder / capsule; with ``meshes`` also <mesh>
    elements -- random convex polytopes, some files holding two objects -- written next to the URDF)."""
    import os
    mesh_no = [0]

    def geom():
        kind = rng.integers(0, 6 if meshes else 4)
        if kind >= 4:
            fn = f"fuzz_mesh_{mesh_no[0]}.obj"
            mesh_no[0] += 1
            random_hull_obj(rng, os.path.join(os.path.dirname(path), fn), n_objects=int(rng.choice([1, 1, 2])), scale=0.08)
            sc = "" if rng.random() < 0.5 else f' scale="{rng.uniform(0.6, 1.4):.3f} {rng.uniform(0.6, 1.4):.3f} {rng.uniform(0.6, 1.4):.3f}"'
            return f'<mesh filename="{fn}"{sc}/>'
        if kind == 0:
            s = rng.uniform(0.04, 0.16, 3)
            return f'<box size="{s[0]:.4f} {s[1]:.4f} {s[2]:.4f}"/>'
        if kind == 1:
            return f'<sphere radius="{rng.uniform(0.02, 0.07):.4f}"/>'
        if kind == 2:
            return f'<cylinder radius="{rng.uniform(0.015, 0.05):.4f}" length="{rng.uniform(0.05, 0.25):.4f}"/>'
        return f'<capsule radius="{rng.uniform(0.015, 0.04):.4f}" length="{rng.uniform(0.05, 0.2):.4f}"/>'

    def origin(scale):
        xyz = rng.uniform(-scale, scale, 3)
        rpy = rng.uniform(-1.0, 1.0, 3) * (rng.random() < 0.6)
        return f'<origin xyz="{xyz[0]:.4f} {xyz[1]:.4f} {xyz[2]:.4f}" rpy="{rpy[0]:.4f} {rpy[1]:.4f} {rpy[2]:.4f}"/>'

    out = ['<?xml version="1.0"?>', '<robot name="fuzz">']
    for i in range(n_links):
        cols = "".join(f"<collision>{origin(0.05)}<geometry>{geom()}</geometry></collision>"
                       for _ in range(int(rng.choice([0, 1, 1, 1, 2]))))
        out.append(f'<link name="l{i}">{cols}</link>')
    for i in range(1, n_links):
        parent = int(rng.integers(max(0, i - max_back), i))
        jt = str(rng.choice(["revolute", "revolute", "continuous", "prismatic", "fixed"]))
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        lim = ""
        if jt == "revolute":
            lim = f'<limit lower="{-rng.uniform(0.5, 3.0):.3f}" upper="{rng.uniform(0.5, 3.0):.3f}" effort="1" velocity="1"/>'
        elif jt == "prismatic":
            lim = f'<limit lower="{-rng.uniform(0.0, 0.1):.3f}" upper="{rng.uniform(0.05, 0.3):.3f}" effort="1" velocity="1"/>'
        axis = "" if jt == "fixed" else f'<axis xyz="{ax[0]:.5f} {ax[1]:.5f} {ax[2]:.5f}"/>'
        out.append(f'<joint name="j{i}" type="{jt}">{origin(0.4)}<parent link="l{parent}"/><child link="l{i}"/>{axis}{lim}</joint>')
    out.append("</robot>")
    with open(path, "w") as f:
        f.write("\n".join(out))
    return path


def random_obstacles(rng, n, reach=0.9, mesh_dir=None):
    """``mesh_dir``: also Mesh obstacles (random polytope files written there; shape kwargs exercised at random)."""
    from geom_truth import random_pose
    from numbotics_amd.physics import Cube, Cuboid, Sphere, Capsule, Cylinder, Plane, Mesh
    import os
    obs = []
    for i in range(n):
        k = int(rng.integers(0, 9 if mesh_dir is not None else 6))
        if k >= 6:
            fn = random_hull_obj(rng, os.path.join(mesh_dir, f"fuzz_obstacle_{i}.obj"), n_objects=int(rng.choice([1, 2, 3])), scale=0.15)
            kw = {}
            if rng.random() < 0.5:
                kw['mesh_scale'] = rng.uniform(0.5, 1.5, 3)
            if rng.random() < 0.5:
                kw['offset'] = random_pose(rng, 0.1)
            if rng.random() < 0.3:
                kw['auto_center'] = True
            if rng.random() < 0.3:
                kw['collision_margin'] = float(rng.choice([0.005, 0.02]))
            obs.append(Mesh(0.0, fn, pose=random_pose(rng, reach), **kw))
            continue
        pose = random_pose(rng, reach)
        margin = float(rng.choice([0.0, 0.0, 0.01, 0.03]))
        if k == 0:
            obs.append(Cube(0.0, float(rng.uniform(0.04, 0.2)), pose=pose))
        elif k == 1:
            obs.append(Cuboid(0.0, rng.uniform(0.05, 0.2, 3), pose=pose, collision_margin=min(margin, 0.04)))
        elif k == 2:
            obs.append(Sphere(0.0, float(rng.uniform(0.03, 0.15)), pose=pose))
        elif k == 3:
            obs.append(Capsule(0.0, float(rng.uniform(0.02, 0.08)), float(rng.uniform(0.1, 0.4)), pose=pose))
        elif k == 4:
            obs.append(Cylinder(0.0, float(rng.uniform(0.04, 0.12)), float(rng.uniform(0.1, 0.3)), pose=pose,
                                collision_margin=min(margin, 0.03)))
        else:
            n_ = rng.normal(size=3)
            n_ /= np.linalg.norm(n_)
            obs.append(Plane(0.0, n_, position=-n_ * float(rng.uniform(0.7, 1.3))))
    return obs


SPEC_AXIS_MODES = ("aligned", "random", "prismatic", "mixed")
WORLD_KINDS = ("sphere", "capsule", "box", "cylinder", "plane", "mesh")          # in the order of the model's shape type codes


def random_spec_robot(rng, path, *, n_joints, n_shapes, axis_mode="mixed", base_shapes=True, fixed_joints=0):
    """A serial chain for the per-robot broadphase: ``n_joints`` moving joints (1-8), ``fixed_joints`` fixed ones (the first at the
    end of the chain, the others between moving joints, never two in a row), exactly ``n_shapes`` collision primitives (1-16) spread
    over the links -- some links empty, some with two or three, the base link (and what is welded to it) with shapes or without.
    ``axis_mode``: "aligned" = exact +-e_x / e_y / e_z revolute axes, "random" = random unit vectors, "prismatic" = prismatic joints
    along random directions, "mixed" = every joint one of the three (each at least once when there are three joints).  Links are short
    (joint offsets 9-15 cm) and shapes sit off their link's origin, so that links meet each other and sweep when their joint turns.
    -> path; the draw order is this function's own (random_urdf is left as it is)."""
    assert 1 <= n_joints <= 32 and n_shapes >= 1 and 0 <= fixed_joints <= n_joints
    # joint sequence: 'm' moving, 'f' fixed
    seq = ['m'] * n_joints
    if fixed_joints > 0:
        gaps = list(rng.permutation(np.arange(1, n_joints)))[:fixed_joints - 1] if n_joints > 1 else []
        for g in sorted((int(g) for g in gaps), reverse=True):
            seq.insert(g, 'f')                       # after at least one moving joint, so the base frame keeps to base_shapes
        seq.append('f')
    n_links = len(seq) + 1
    # shapes per link: the base gets 1-2 or none; the rest dealt at random with at most three per link
    counts = np.zeros(n_links, dtype=int)
    first = 1
    if base_shapes and n_shapes > 1:
        counts[0] = min(int(rng.integers(1, 3)), n_shapes - 1)
    elif base_shapes:
        counts[0] = 1
    left = n_shapes - int(counts[0])
    assert left <= 3 * (n_links - first), "too many shapes for this many links"
    if left > 0:
        counts[n_links - 1 if seq[-1] == 'm' else n_links - 2] = 1           # the last moving frame is never empty (J stays n_joints)
        left -= 1
    while left > 0:
        i = int(rng.integers(first, n_links))
        if counts[i] < 3 and (counts[i] > 0 or rng.random() < 0.6):          # keeps some links empty while others fill up
            counts[i] += 1
            left -= 1

    def geom():
        kind = int(rng.integers(0, 4))
        if kind == 0:
            s = rng.uniform(0.05, 0.1, 3)
            return f'<box size="{s[0]:.4f} {s[1]:.4f} {s[2]:.4f}"/>'
        if kind == 1:
            return f'<sphere radius="{rng.uniform(0.03, 0.055):.4f}"/>'
        if kind == 2:
            return f'<cylinder radius="{rng.uniform(0.025, 0.045):.4f}" length="{rng.uniform(0.05, 0.11):.4f}"/>'
        return f'<capsule radius="{rng.uniform(0.02, 0.04):.4f}" length="{rng.uniform(0.04, 0.1):.4f}"/>'

    def origin(lo, hi):
        d = rng.normal(size=3)
        xyz = d / np.linalg.norm(d) * rng.uniform(lo, hi)
        rpy = rng.uniform(-1.0, 1.0, 3) * (rng.random() < 0.6)
        return f'<origin xyz="{xyz[0]:.4f} {xyz[1]:.4f} {xyz[2]:.4f}" rpy="{rpy[0]:.4f} {rpy[1]:.4f} {rpy[2]:.4f}"/>'

    modes = []
    for k in range(n_joints):
        modes.append(axis_mode if axis_mode != "mixed" else SPEC_AXIS_MODES[int(rng.integers(0, 3))])
    if axis_mode == "mixed" and n_joints >= 3:
        for k, mname in zip(rng.permutation(n_joints)[:3], SPEC_AXIS_MODES[:3]):
            modes[int(k)] = mname
    out = ['<?xml version="1.0"?>', '<robot name="spec_fuzz">']
    for i in range(n_links):
        cols = "".join(f"<collision>{origin(0.02, 0.06)}<geometry>{geom()}</geometry></collision>" for _ in range(int(counts[i])))
        out.append(f'<link name="l{i}">{cols}</link>')
    k = 0
    for i in range(1, n_links):
        head = f'{origin(0.09, 0.15)}<parent link="l{i - 1}"/><child link="l{i}"/>'
        if seq[i - 1] == 'f':
            out.append(f'<joint name="j{i}" type="fixed">{head}</joint>')
            continue
        mode = modes[k]
        k += 1
        if mode == "aligned":
            ax = np.zeros(3)
            ax[int(rng.integers(0, 3))] = float(rng.choice([-1.0, 1.0]))
            axis = f'<axis xyz="{ax[0]:.0f} {ax[1]:.0f} {ax[2]:.0f}"/>'
        else:
            ax = rng.normal(size=3)
            ax /= np.linalg.norm(ax)
            axis = f'<axis xyz="{ax[0]:.5f} {ax[1]:.5f} {ax[2]:.5f}"/>'
        if mode == "prismatic":
            jt, lim = "prismatic", f'<limit lower="{-rng.uniform(0.05, 0.2):.3f}" upper="{rng.uniform(0.05, 0.25):.3f}" effort="1" velocity="1"/>'
        elif rng.random() < 0.3:
            jt, lim = "continuous", ""
        else:
            jt, lim = "revolute", f'<limit lower="{-rng.uniform(1.5, 3.1):.3f}" upper="{rng.uniform(1.5, 3.1):.3f}" effort="1" velocity="1"/>'
        out.append(f'<joint name="j{i}" type="{jt}">{head}{axis}{lim}</joint>')
    out.append("</robot>")
    with open(path, "w") as f:
        f.write("\n".join(out))
    return path


def spec_obstacles(rng, kinds, reach, mesh_dir=None, first=0):
    """One obstacle per entry of ``kinds`` (names from WORLD_KINDS; "mesh" needs ``mesh_dir``), named obs<first>, obs<first + 1>, ... so
    that the scene model lists them in this order, each placed inside ``reach`` of the base but clear of the base link's own shapes."""
    import os
    from geom_truth import random_pose
    from numbotics_amd.physics import Cuboid, Sphere, Capsule, Cylinder, Plane, Mesh
    obs = []
    for i, kind in enumerate(kinds, start=first):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        pose = random_pose(rng, 0.0)
        pose[:3, 3] = d * rng.uniform(0.55, 0.85) * reach
        name = f"obs{i}"
        if kind == "sphere":
            obs.append(Sphere(0.0, float(rng.uniform(0.05, 0.09)), pose=pose, name=name))
        elif kind == "capsule":
            obs.append(Capsule(0.0, float(rng.uniform(0.035, 0.06)), float(rng.uniform(0.08, 0.2)), pose=pose, name=name))
        elif kind == "box":
            obs.append(Cuboid(0.0, rng.uniform(0.04, 0.09, 3), pose=pose, name=name,
                              **({'collision_margin': 0.01} if rng.random() < 0.3 else {})))
        elif kind == "cylinder":
            obs.append(Cylinder(0.0, float(rng.uniform(0.04, 0.08)), float(rng.uniform(0.08, 0.2)), pose=pose, name=name))
        elif kind == "plane":
            obs.append(Plane(0.0, d, position=-d * float(rng.uniform(0.35, 0.7)) * reach, name=name))
        elif kind == "mesh":
            fn = random_hull_obj(rng, os.path.join(mesh_dir, f"spec_obstacle_{i}.obj"), n_objects=1, scale=0.09)
            obs.append(Mesh(0.0, fn, pose=pose, name=name))
        else:
            raise ValueError(kind)
    return obs
