"""mbrl_amd -- MI355X-native MPC/CEM planning hot path of Khodeir/mujoco-mbrl.

Drop-in for the reference's planner API (src/mbrl/planners.py) and DynamicsModel.forward
(src/mbrl/models.py); the compute runs in the in-tree HIP extension libmbrl_cem.so (C ABI:
include/mbrl_cem.h). See DESIGN.md and INTEGRATION.md at the repository root.
"""
from . import agents, data, device_data, env, env_wrappers, gd, models, parallel, planners  # noqa: F401
from .agents import MPCPolicy  # noqa: F401
from .device_data import DeviceTransitionsDataset  # noqa: F401
from .env_wrappers import EnvWrapper  # noqa: F401
from .models import (CoshLoss, CostModel, DynamicsModel, EnsembleModel, LinearModel, Model,  # noqa: F401
                     ModelWithReward, QuadraticCost, SmoothAbsLoss, compose, goal_state_cost, member_order,
                     state_action_cost)
from .planners import (BatchedMPPIPlanner, CEMPlanner, GradientDescentPlanner, ModelPlanner, MPPIPlanner,  # noqa: F401
                       RandomShootingPlanner, RecedingHorizonCEMPlanner, TrajectorySamplingCEMPlanner,
                       cem_plan_batch_rh, cem_shift_carry, mppi_plan_batch)


def load_extension():
    """Load the HIP extension now (raises ImportError if it is not built)."""
    from . import _lib
    return _lib.load()
