__all__ = ['unit_bspline', 'unit_knots', 'collision_mask', 'counter_example_bisection']

from .trajectories import unit_bspline, unit_knots
from .safe_sets import collision_mask, counter_example_bisection
