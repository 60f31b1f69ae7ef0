"""Argument checks of the pair-subset entry points (Arm.pair_proximity_jacobians, item_proximity_jacobians,
closest_proximity_jacobians): shapes and pair indices are validated against scene_model() before anything touches the
device, so the errors are the same with or without a GPU.  No GPU needed."""
import numpy as np
import pytest

from numbotics_amd.scenes import build_scene


def test_the_new_symbol_is_declared_and_registered():
    from numbotics_amd import _lib
    assert "nbk_pair_records_items" in _lib.SYMBOLS
    assert hasattr(_lib.load(), "nbk_pair_records_items")


def test_pair_indices_and_shapes_are_checked_on_the_host(fresh_world):
    arm, chain, obs = build_scene("c2")
    P = arm.scene_model().n_pairs
    assert P > 0
    q = np.zeros((5, arm.dof))
    for bad in ([P], [-1], [0, P + 3], [[0, 1]], [0.5], [True]):
        with pytest.raises(ValueError):
            arm.pair_proximity_jacobians(q, bad)
    with pytest.raises(ValueError):
        arm.pair_proximity_jacobians(np.zeros((5, arm.dof + 1)), [0])
    with pytest.raises(ValueError):
        arm.item_proximity_jacobians(q, np.array([0, 1, 2, 3, P]))       # out of range
    with pytest.raises(ValueError):
        arm.item_proximity_jacobians(q, np.array([0, 1, 2, 3, -1]))
    with pytest.raises(ValueError):
        arm.item_proximity_jacobians(q, np.array([0, 1, 2]))             # one pair per configuration
    with pytest.raises(ValueError):
        arm.item_proximity_jacobians(q, np.zeros(5))                     # not integers
    with pytest.raises(ValueError):
        arm.item_proximity_jacobians(np.zeros((5, arm.dof - 1)), np.zeros(5, dtype=np.int64))
    with pytest.raises(ValueError):
        arm.closest_proximity_jacobians(np.zeros((5, arm.dof + 2)))


def test_closest_records_need_pairs(fresh_world):
    arm, chain, obs = build_scene("c2")
    for a, b in list(arm.collision_pairs()):
        arm.remove_collision_pair(a, b)
    assert arm.scene_model().n_pairs == 0
    with pytest.raises(ValueError, match="empty sequence"):
        arm.closest_proximity_jacobians(np.zeros((3, arm.dof)))
