"""MI355X-native batched LPV-MPC / LPV-MPP solve path (drop-in for the reference's
PathFollowingLPV_MPC / LPV_MPC_Planner classes).  Import as ``lpvmpc`` (alias package at the repo root)
or via ``importlib.import_module("autonomous-racing-lpv-mpp-mpc_amd")``."""
from .api import (BatchedSolver, LPV_MPC_Planner, PathFollowingLPV_MPC, PlannerHandoff, RaceFleet,  # noqa: F401
                  body_frame_errors, handoff_operators, observer_design_config)
from ._ffi import LpvMpcError, STATUS_TEXT  # noqa: F401
from .observer import GainScheduledLPVObserver, observer_config, observer_vertex_gains  # noqa: F401
from .track import Map  # noqa: F401
from .actuator import actuator_config, controller_delay, delay_steps  # noqa: F401
from .plant import plant_params, sample_plant_params, sample_tyre_params, tyre_params  # noqa: F401
from .model import model_params, sample_model_params  # noqa: F401
from .tuning import check_tuning_rows, sample_tunings, tuning_rows  # noqa: F401
from .disturbance import check_disturbance_rows, disturbance_rows, rho_from_tau, sample_disturbances  # noqa: F401
from .sensor_faults import check_fault_rows, fault_rows, sample_faults  # noqa: F401
from .snapshot import RaceSnapshot, respawn_sources  # noqa: F401
from .tyre_wear import check_tyre_wear_rows, sample_tyre_wear, tyre_wear_rows  # noqa: F401

__all__ = ["BatchedSolver", "PathFollowingLPV_MPC", "LPV_MPC_Planner", "PlannerHandoff", "body_frame_errors", "handoff_operators",
           "Map", "LpvMpcError", "STATUS_TEXT", "GainScheduledLPVObserver", "observer_config", "observer_vertex_gains", "RaceFleet",
           "actuator_config", "controller_delay", "delay_steps", "plant_params", "sample_plant_params", "tyre_params", "sample_tyre_params",
           "model_params", "sample_model_params", "tuning_rows", "sample_tunings", "check_tuning_rows",
           "disturbance_rows", "sample_disturbances", "check_disturbance_rows", "rho_from_tau",
           "tyre_wear_rows", "sample_tyre_wear", "check_tyre_wear_rows",
           "fault_rows", "sample_faults", "check_fault_rows",
           "RaceSnapshot", "respawn_sources"]
