"""Importable alias of the package directory ``autonomous-racing-lpv-mpp-mpc_amd/`` (whose name is not a
valid Python identifier).  All code lives there; this file only points ``__path__`` at it."""
import os as _os

__path__ = [_os.path.join(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))),
                          "autonomous-racing-lpv-mpp-mpc_amd")]

from .api import (BatchedSolver, LPV_MPC_Planner, PathFollowingLPV_MPC, PlannerHandoff, RaceFleet,  # noqa: E402,F401
                  body_frame_errors, handoff_operators)
from ._ffi import LpvMpcError, STATUS_TEXT  # noqa: E402,F401
from .observer import GainScheduledLPVObserver, observer_config, observer_vertex_gains  # noqa: E402,F401
from .track import Map  # noqa: E402,F401
from .actuator import actuator_config, controller_delay, delay_steps  # noqa: E402,F401
from .plant import plant_params, sample_plant_params, sample_tyre_params, tyre_params  # noqa: E402,F401
from .model import model_params, sample_model_params  # noqa: E402,F401
from .tuning import check_tuning_rows, sample_tunings, tuning_rows  # noqa: E402,F401
from .disturbance import check_disturbance_rows, disturbance_rows, rho_from_tau, sample_disturbances  # noqa: E402,F401
from .sensor_faults import check_fault_rows, fault_rows, sample_faults  # noqa: E402,F401
from .snapshot import RaceSnapshot, respawn_sources  # noqa: E402,F401
from .tyre_wear import check_tyre_wear_rows, sample_tyre_wear, tyre_wear_rows  # noqa: E402,F401

__all__ = ["BatchedSolver", "PathFollowingLPV_MPC", "LPV_MPC_Planner", "PlannerHandoff", "body_frame_errors", "handoff_operators",
           "Map", "LpvMpcError", "STATUS_TEXT", "GainScheduledLPVObserver", "observer_config", "observer_vertex_gains", "RaceFleet",
           "actuator_config", "controller_delay", "delay_steps", "plant_params", "sample_plant_params", "tyre_params", "sample_tyre_params",
           "model_params", "sample_model_params", "tuning_rows", "sample_tunings", "check_tuning_rows",
           "disturbance_rows", "sample_disturbances", "check_disturbance_rows", "rho_from_tau",
           "tyre_wear_rows", "sample_tyre_wear", "check_tyre_wear_rows",
           "fault_rows", "sample_faults", "check_fault_rows",
           "RaceSnapshot", "respawn_sources"]
