"""Inputs of tests/test_gpu_ca_keys.py: the smallest batches on which the keys of a certified call ("the key of a
certified call") can go wrong -- an edge that collides at t = 0 (key 0) beside a degenerate one, both reserved keys, and more than
one 256-thread block of the init and final kernels.  tests/test_ca_keys_host.py asserts the composition on the CPU."""
import numpy as np

from numbotics_amd.scenes import build_scene
from cloud_cases import scan
from continuous_ref import random_edges
from spline_continuous_ref import spline_from_edges

MAX_DISTANCE = {"connect": 10.0, "steer": 0.6}
MAX_ITERS = (64, 1)
TILES = 4                       # 66 edges -> 264, 67 splines -> 268: both cross a 256-thread block
CLOUD_R = 0.01
CLOUD_BOX = ([-0.6, -0.6, 0.0], [0.6, 0.6, 1.0])
CLOUD_LOOK_AHEAD = 0.1         # long enough that most free edges finish within 64 steps, short enough that the D_cap exit is taken
N_KEPT = 10                     # rows of the hand-made `out` that come in as the world guard leaves them


def scene():
    return build_scene("c2", bullet_margins=True)


def edges(chain):
    """64 random edges and two degenerate ones (rows 64, 65)."""
    s, g = random_edges(chain, 64, 7, scale=0.35)
    return np.concatenate((s, s[:2])), np.concatenate((g, s[:2] + 1e-9))


def splines(chain):
    """The 64 edges as cubic splines of 4 control points, then one whose control points are all equal, one with a NaN and one with
    an inf control point (rows 64, 65, 66)."""
    s, g = random_edges(chain, 64, 7, scale=0.35)
    c = spline_from_edges(s, g, n=4, k=3)
    extra = c[:3].copy()
    extra[0, :] = extra[0, 0]
    extra[1, 2, 1] = np.nan
    extra[2, 1, 0] = np.inf
    return np.concatenate((c, extra))


def unclamped_knots():
    return np.array([0.0, 0.0, 0.0, 0.1, 1.0, 1.0, 1.0, 1.0])


def cloud(sm):
    """48 points of the scan and the last three robot shapes."""
    return np.ascontiguousarray(scan(48, seed=48)), list(range(sm.n_rshapes - 3, sm.n_rshapes))


def tiled(a, times=TILES):
    return np.concatenate([a] * times)
