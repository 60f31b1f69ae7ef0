"""Scenes of the broadphase-trim tests (test_broad_trim_source.py on the CPU, test_gpu_broad_trim.py on the GPU): c2 and variants of it
whose world boxes are, or are not, axis-aligned, as SceneModels; built the same way in every process."""
import dataclasses

import numpy as np

import spec_cases as sc

SCENES = ("c2", "c2_sharp", "c2_rot", "plane_hull", "two_box")
# wbox_aligned of the generated Spec, per listed world shape
ALIGNED = {"c2": [1], "c2_sharp": [1], "c2_rot": [0], "plane_hull": [0, 0], "two_box": [1, 0]}
WORLD_RADIUS = 4.0


def rot_z(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def with_pose(sm, w, R=None, t=None):
    """``sm`` with world shape ``w`` rotated to ``R`` and / or moved to ``t``."""
    P = sm.wshape_pose.reshape(-1, 3, 4).copy()
    if R is not None:
        P[w, :, :3] = R
    if t is not None:
        P[w, :, 3] = t
    return dataclasses.replace(sm, wshape_pose=np.ascontiguousarray(P.reshape(-1, 12)))


def scene(name):
    """-> (SceneModel, chain) of one named scene in a fresh world."""
    from numbotics_amd.scenes import build_scene
    if name == "plane_hull":
        arm, chain, obs = sc.named_case(name)
        return arm.scene_model(), chain
    sc.fresh()
    arm, chain, obs = build_scene("c2", bullet_margins=name != "c2_sharp")
    if name == "two_box":
        from numbotics_amd.physics import Cube
        obs.append(Cube(half_extent=0.15, mass=0.0, position=np.array([0.45, -0.35, 0.85])))
    sm = arm.scene_model()
    if name == "c2_rot":
        sm = with_pose(sm, 0, R=rot_z(0.3))
    if name == "two_box":
        sm = with_pose(sm, 1, R=rot_z(0.3))
    return sm, chain
