"""ctypes binding of liblpvmpc.so (C ABI in include/lpvmpc.h).

There is no CPU fallback: if the shared library is missing this module raises at load time, and if no
HIP device is usable ``lpvmpc_create`` fails with LPVMPC_E_NODEVICE which surfaces as ``LpvMpcError``.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblpvmpc.so")

KIND_CONTROLLER, KIND_PLANNER = 0, 1
MAX_TRACK_ROWS, MAX_N = 16, 52
E_ARG, E_NODEVICE, E_HIP, E_NOMEM = -1, -2, -3, -4

STATUS_TEXT = {1: "solved", 2: "solved inaccurate", 3: "primal infeasible inaccurate",
               4: "dual infeasible inaccurate", -2: "maximum iterations reached",
               -3: "primal infeasible", -4: "dual infeasible", -7: "problem non convex", -10: "unsolved"}

_d, _i = C.c_double, C.c_int32


class Config(C.Structure):
    """Mirror of ``struct lpvmpc_config`` (include/lpvmpc.h) -- keep field order identical."""
    _fields_ = [
        ("kind", _i), ("N", _i), ("device", _i), ("steering_delay", _i),
        ("dt", _d),
        ("lf", _d), ("lr", _d), ("m", _d), ("Iz", _d), ("Cf", _d), ("Cr", _d), ("mu", _d),
        ("max_vel", _d), ("min_vel", _d),
        ("Q", _d * 36), ("R", _d * 4), ("dR", _d * 2), ("L_cf", _d * 6),
        ("ctrl_vx_min", _d), ("ctrl_delta_max", _d), ("ctrl_a_max", _d), ("ctrl_a_min_abs", _d),
        ("plan_xmin", _d * 5), ("plan_xmax", _d * 5), ("plan_umin", _d * 2), ("plan_umax", _d * 2),
        ("rho", _d), ("sigma", _d), ("alpha", _d), ("eps_abs", _d), ("eps_rel", _d),
        ("eps_prim_inf", _d), ("eps_dual_inf", _d), ("polish_delta", _d), ("adaptive_rho_tolerance", _d),
        ("max_iter", _i), ("check_termination", _i), ("scaling", _i), ("adaptive_rho", _i),
        ("adaptive_rho_interval", _i), ("polish", _i), ("polish_refine_iter", _i), ("reserved1", _i),
        ("track_rows", _i), ("reserved2", _i),
        ("track", _d * (MAX_TRACK_ROWS * 6)),
    ]


SETTING_FIELDS = ("rho", "sigma", "alpha", "eps_abs", "eps_rel", "eps_prim_inf", "eps_dual_inf", "polish_delta",
                  "adaptive_rho_tolerance", "max_iter", "check_termination", "scaling", "adaptive_rho",
                  "adaptive_rho_interval", "polish", "polish_refine_iter",
                  "ctrl_vx_min", "ctrl_delta_max", "ctrl_a_max", "ctrl_a_min_abs", "steering_delay",
                  "plan_xmin", "plan_xmax", "plan_umin", "plan_umax")


class LpvMpcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("lpvmpc error %d: %s" % (code, msg))
        self.code = code


MAX_FILTER_ORDER = 8


class HandoffConfig(C.Structure):
    """Mirror of ``struct lpvmpc_handoff_config`` (include/lpvmpc.h)."""
    _fields_ = [("interp_dt", _d), ("padlen", _i), ("order", _i), ("b", _d * (MAX_FILTER_ORDER + 1)), ("a", _d * (MAX_FILTER_ORDER + 1))]


class ObserverConfig(C.Structure):
    """Mirror of ``struct lpvmpc_observer_config`` (include/lpvmpc.h)."""
    _fields_ = [("L_ls", _d * 480), ("lim_ls", _d * 12), ("L_hs", _d * 480), ("lim_hs", _d * 12),
                ("loop_rate", _d), ("init_vx", _d), ("psi_std", _d), ("psiDot_std", _d), ("x_std", _d), ("y_std", _d),
                ("v_std", _d), ("n_bound", _d), ("gps_freq", _d), ("seed", C.c_uint64), ("vehicle_offset", C.c_int64)]


class ObserverDesign(C.Structure):
    """Mirror of ``struct lpvmpc_observer_design`` (include/lpvmpc.h)."""
    _fields_ = [("lim_ls", _d * 12), ("lim_hs", _d * 12), ("Qo", _d * 36), ("Ro", _d * 25)]


class RaceConfig(C.Structure):
    """Mirror of ``struct lpvmpc_race_config`` (include/lpvmpc.h)."""
    _fields_ = [("laps", _i), ("n_sub_lap0", _i), ("n_sub", _i * 3), ("q9_swap", _i), ("half_width", _d), ("slack", _d),
                ("plan_max_ey", _d), ("dt_sim", _d), ("mu_sim", _d)]


class ActuatorConfig(C.Structure):
    """Mirror of ``struct lpvmpc_actuator_config`` (include/lpvmpc.h)."""
    _fields_ = [("delay_a", _i), ("delay_df", _i), ("low_level_dyn", _i), ("reserved", _i), ("servo_tf", _d)]


class DisturbanceConfig(C.Structure):
    """Mirror of ``struct lpvmpc_disturbance_config`` (include/lpvmpc.h)."""
    _fields_ = [("seed", C.c_uint64), ("vehicle_offset", C.c_int64), ("n_bound", _d)]


class SensorFaultConfig(C.Structure):
    """Mirror of ``struct lpvmpc_sensor_fault_config`` (include/lpvmpc.h)."""
    _fields_ = [("seed", C.c_uint64), ("vehicle_offset", C.c_int64)]


class RaceRecordConfig(C.Structure):
    """Mirror of ``struct lpvmpc_race_record_config`` (include/lpvmpc.h)."""
    _fields_ = [("capacity", _i), ("stride", _i)]


class HeatsConfig(C.Structure):
    """Mirror of ``struct lpvmpc_heats_config`` (include/lpvmpc.h)."""
    _fields_ = [("half_length", _d), ("half_width_car", _d)]


# heats (LPVMPC_HEAT_*): standings f64 [HEAT_F64][B] / i32 [HEAT_I32][B] and the carried state of the batch form, named in channel order
HEAT_MAX = 256
HEAT_F64, HEAT_I32, HEAT_CARRY_F64, HEAT_CARRY_I32 = 5, 10, 3, 10
HEAT_F64_NAMES = ("progress", "gap_ahead", "gap_leader", "clearance", "min_clearance")
HEAT_I32_NAMES = ("position", "ahead", "nearest", "contact", "contact_ticks", "first_contact_tick", "passes", "passed", "turns", "class")
HEAT_CARRY_F64_NAMES = ("s", "progress", "min_clearance")
HEAT_CARRY_I32_NAMES = ("flags", "turns", "turns0", "crossings", "phase", "finish_tick", "contact_ticks", "first_contact_tick", "passes",
                        "passed")


class InteractionConfig(C.Structure):
    """Mirror of ``struct lpvmpc_interaction_config`` (include/lpvmpc.h)."""
    _fields_ = [("draft_gain", _d), ("wake_length", _d), ("wake_half_width", _d), ("contact", _i), ("reserved", _i), ("restitution", _d),
                ("push", _d)]


# interactions (LPVMPC_INTER_*): outputs f64 [INTER_F64][B] / i32 [INTER_I32][B] and the carried state of the batch form, in channel order
INTER_F64, INTER_I32, INTER_CARRY_F64, INTER_CARRY_I32 = 4, 5, 1, 3
INTER_F64_NAMES = ("shelter", "mu", "impulse", "impulse_total")
INTER_I32_NAMES = ("leader", "hit", "hit_ticks", "first_hit_tick", "draft_ticks")
INTER_CARRY_F64_NAMES = ("impulse_total",)
INTER_CARRY_I32_NAMES = ("hit_ticks", "first_hit_tick", "draft_ticks")


class WallConfig(C.Structure):
    """Mirror of ``struct lpvmpc_wall_config`` (include/lpvmpc.h)."""
    _fields_ = [("margin", _d), ("reach", _d), ("half_length", _d), ("half_width_car", _d), ("restitution", _d), ("friction", _d), ("push", _d),
                ("yaw_response", _i), ("reserved", _i)]


# walls (LPVMPC_WALL_*): outputs f64 [WALL_F64][B] / i32 [WALL_I32][B] and the carried state of the batch form, in channel order
WALL_F64, WALL_I32, WALL_CARRY_F64, WALL_CARRY_I32 = 4, 6, 2, 2
WALL_F64_NAMES = ("depth", "impulse", "impulse_total", "max_impulse")
WALL_I32_NAMES = ("hit", "side", "corner", "hit_ticks", "first_hit_tick", "outside")
WALL_CARRY_F64_NAMES = ("impulse_total", "max_impulse")
WALL_CARRY_I32_NAMES = ("hit_ticks", "first_hit_tick")


class ContactConfig(C.Structure):
    """Mirror of ``struct lpvmpc_contact_config`` (include/lpvmpc.h)."""
    _fields_ = [("friction", _d), ("yaw_response", _i), ("reserved", _i)]


# contact model (LPVMPC_CONTACT_*): planes f64 [CONTACT_F64][B] / i32 [CONTACT_I32][B] and the carried state of the batch form
CONTACT_F64, CONTACT_I32, CONTACT_CARRY_F64, CONTACT_CARRY_I32 = 3, 2, 1, 1
CONTACT_F64_NAMES = ("friction_impulse", "yaw_kick", "yaw_kick_total")
CONTACT_I32_NAMES = ("partners", "max_partners")
CONTACT_CARRY_F64_NAMES = ("yaw_kick_total",)
CONTACT_CARRY_I32_NAMES = ("max_partners",)


class EventConfig(C.Structure):
    """Mirror of ``struct lpvmpc_event_config`` (include/lpvmpc.h)."""
    _fields_ = [("capacity", _i), ("kinds", C.c_uint32), ("reserved", _i * 2)]


# race event log (LPVMPC_EVENT_*): an event's words i32 [EVENT_I32] / f64 [EVENT_F64], the kinds, the per-vehicle outputs and the carried
# state of the batch form, in channel order
EVENT_I32, EVENT_F64, EVENT_OUT_I32, EVENT_CARRY_F64, EVENT_CARRY_I32 = 6, 2, 2, 2, 11
EVENT_I32_NAMES = ("tick", "kind", "vehicle", "other", "a", "b")
EVENT_F64_NAMES = ("v0", "v1")
EVENT_KIND_NAMES = ("lap", "finish", "lost", "pass", "contact_begin", "contact_end", "wall_hit", "wall_clear")     # kinds 1 .. 8
EVENT_ALL_KINDS = 0x1FE
EVENT_OUT_I32_NAMES = ("count", "count_total")
EVENT_CARRY_F64_NAMES = ("min_clearance", "max_impulse")
EVENT_CARRY_I32_NAMES = ("flags", "phase", "lap", "position", "class", "contact", "nearest", "contact_start", "hit", "hit_start", "count_total")


# race recorder channels (LPVMPC_REC_*): f64 [REC_F64][B] and i32 [REC_I32][B] per record, named in channel order
REC_F64, REC_I32 = 29, 8
REC_PLANT, REC_LOCAL, REC_CMD, REC_REF, REC_TRACK, REC_EST = 0, 8, 14, 16, 20, 23
REC_PHASE, REC_LAP, REC_SRC, REC_ITERS, REC_STATUS, REC_PLAN_ITERS, REC_PLAN_STATUS, REC_INSIDE = range(8)
REC_F64_NAMES = ("x", "y", "vx", "vy", "ax", "ay", "yaw", "psiDot",
                 "local_vx", "local_vy", "local_w", "local_epsi", "local_s", "local_ey",
                 "servo", "motor", "x_ref", "y_ref", "yaw_ref", "vel_ref", "track_s", "track_ey", "track_epsi",
                 "est_vx", "est_vy", "est_psiDot", "est_x", "est_y", "est_yaw")
REC_I32_NAMES = ("phase", "lap", "src", "iters", "status", "plan_iters", "plan_status", "inside")
# per-lap statistics (LPVMPC_LAPSTAT_*): [B][laps + 1][K]
LAPSTAT_F64, LAPSTAT_I32 = 6, 9
LAPSTAT_SSE_V, LAPSTAT_SSE_EY, LAPSTAT_SSE_EPSI, LAPSTAT_MAX_EY, LAPSTAT_SUM_VX, LAPSTAT_MAX_EY_TRACK = range(6)
(LAPSTAT_TICKS, LAPSTAT_CTRL_ITERS, LAPSTAT_CTRL_ITERS_MAX, LAPSTAT_CTRL_NOT_SOLVED, LAPSTAT_PLAN_TICKS, LAPSTAT_PLAN_ITERS,
 LAPSTAT_PLAN_ITERS_MAX, LAPSTAT_PLAN_NOT_SOLVED, LAPSTAT_OFF_TRACK) = range(9)
LAPSTAT_F64_NAMES = ("sse_v", "sse_ey", "sse_epsi", "max_ey", "sum_vx", "max_ey_track")
LAPSTAT_I32_NAMES = ("ticks", "ctrl_iters", "ctrl_iters_max", "ctrl_not_solved", "plan_ticks", "plan_iters", "plan_iters_max",
                     "plan_not_solved", "off_track")


def lap_stats_dict(f, i, end_tick):
    """Per-lap statistics planes f [B, laps+1, LAPSTAT_F64], i [B, laps+1, LAPSTAT_I32] -> dict of named [B, laps+1] arrays, the
    planes themselves (f64, i32) and end_tick [B]."""
    out = {k: f[:, :, c] for c, k in enumerate(LAPSTAT_F64_NAMES)}
    out.update({k: i[:, :, c] for c, k in enumerate(LAPSTAT_I32_NAMES)})
    out.update(f64=f, i32=i, end_tick=end_tick)
    return out


ACT_MAX_DELAY = 64                       # LPVMPC_ACT_MAX_DELAY
ACT_WORDS = 2 * ACT_MAX_DELAY + 2        # LPVMPC_ACT_WORDS: [motor ring, servo ring, servo_inp, k] per vehicle

PLANT_WORDS = 7                          # LPVMPC_PLANT_WORDS: [lf, lr, m, Iz, Cf, Cr, mu] per vehicle
PLANT_WORD_NAMES = ("lf", "lr", "m", "Iz", "Cf", "Cr", "mu")
TYRE_WORDS = 4                           # LPVMPC_TYRE_WORDS: [kind, B, C, c_f] per vehicle (plant.py, "tyre rows")
TYRE_WORD_NAMES = ("kind", "B", "C", "c_f")
DIST_WORDS, DIST_STATE = 13, 5           # LPVMPC_DIST_WORDS, LPVMPC_DIST_STATE (disturbance.py)
DIST_STREAM = 0xD157A2B3C4D5E6F7         # LPVMPC_DIST_STREAM
WEAR_WORDS, WEAR_STATE = 12, 6           # LPVMPC_WEAR_WORDS, LPVMPC_WEAR_STATE (tyre_wear.py)
FAULT_WORDS, OBS_STATE_WORDS = 12, 18    # LPVMPC_FAULT_WORDS, LPVMPC_OBS_STATE_WORDS (sensor_faults.py)
FAULT_STREAM = 0x5E4507FA17C0FFEE        # LPVMPC_FAULT_STREAM
MODEL_WORDS = 7                          # LPVMPC_MODEL_WORDS: the same words, as a controller's / planner's model of the vehicle
MAX_TRACKS = 64                          # LPVMPC_MAX_TRACKS: entries of a track palette (track.pack_tracks)
TUNING_WORDS = 64                        # LPVMPC_TUNING_WORDS: Q[36] R[4] dR[2] L_cf[6] limits[16] per instance (tuning.py)

OBSERVER_AUX = 30 + 36 + 12      # L_gain [6][5], A_obs [6][6], B_obs [6][2] per instance (lpvmpc_observer_step_batch)

EXPORTS = ("lpvmpc_version", "lpvmpc_default_config", "lpvmpc_create", "lpvmpc_destroy", "lpvmpc_last_error", "lpvmpc_last_error_code",
           "lpvmpc_reserve", "lpvmpc_lpv_batch", "lpvmpc_estimate_abc_batch", "lpvmpc_solve_batch_AB",
           "lpvmpc_solve_batch", "lpvmpc_solve_batch_dev", "lpvmpc_last_kernel_ms", "lpvmpc_set_timing",
           "lpvmpc_kernel_time_stats", "lpvmpc_set_option",
           "lpvmpc_local_position_batch", "lpvmpc_global_position_batch", "lpvmpc_plant_step_batch",
           "lpvmpc_cl_init", "lpvmpc_cl_tick", "lpvmpc_cl_read", "lpvmpc_cl_release", "lpvmpc_join", "lpvmpc_resume_time_stats", "lpvmpc_defer_stats",
           "lpvmpc_handoff_default_config", "lpvmpc_handoff_length", "lpvmpc_handoff_operators", "lpvmpc_handoff_setup",
           "lpvmpc_handoff_batch", "lpvmpc_cascade_init", "lpvmpc_cascade_tick", "lpvmpc_cascade_read", "lpvmpc_cascade_alive_ticks",
           "lpvmpc_observer_default_config", "lpvmpc_observer_setup", "lpvmpc_observer_read", "lpvmpc_observer_step_batch",
           "lpvmpc_solve_batch_masked", "lpvmpc_race_default_config", "lpvmpc_race_init", "lpvmpc_race_tick", "lpvmpc_race_read",
           "lpvmpc_race_laps", "lpvmpc_race_predictions", "lpvmpc_race_init_observed",
           "lpvmpc_actuator_default_config", "lpvmpc_plant_step_actuated_batch", "lpvmpc_cl_init_actuated", "lpvmpc_race_init_actuated",
           "lpvmpc_actuator_read", "lpvmpc_race_record", "lpvmpc_race_record_read", "lpvmpc_race_lap_stats",
           "lpvmpc_plant_step_vehicles_batch", "lpvmpc_cl_init_vehicles", "lpvmpc_race_init_vehicles", "lpvmpc_plant_params_read",
           "lpvmpc_set_model_params", "lpvmpc_model_params_read",
           "lpvmpc_set_tunings", "lpvmpc_tunings_read", "lpvmpc_tuning_from_config", "lpvmpc_tuning_device_row",
           "lpvmpc_plant_step_tyres_batch", "lpvmpc_cl_init_tyres", "lpvmpc_race_init_tyres", "lpvmpc_tyre_params_read",
           "lpvmpc_tyre_force_batch",
           "lpvmpc_observer_default_design", "lpvmpc_observer_design_batch", "lpvmpc_set_observer_vehicles",
           "lpvmpc_observer_vehicles_read", "lpvmpc_observer_step_vehicles_batch",
           "lpvmpc_set_tracks", "lpvmpc_tracks_read",
           "lpvmpc_disturbance_default_config", "lpvmpc_set_disturbances", "lpvmpc_disturbances_read",
           "lpvmpc_plant_step_disturbed_batch",
           "lpvmpc_set_tyre_wear", "lpvmpc_tyre_wear_read", "lpvmpc_tyre_wear_fit", "lpvmpc_plant_step_worn_batch",
           "lpvmpc_race_snapshot_size", "lpvmpc_race_snapshot", "lpvmpc_race_restore", "lpvmpc_race_clone",
           "lpvmpc_heats_default_config", "lpvmpc_race_heats", "lpvmpc_race_standings", "lpvmpc_heat_step_batch",
           "lpvmpc_sensor_fault_default_config", "lpvmpc_set_sensor_faults", "lpvmpc_sensor_faults_read", "lpvmpc_sensor_step_batch",
           "lpvmpc_interaction_default_config", "lpvmpc_race_interactions", "lpvmpc_race_interactions_read", "lpvmpc_interaction_step_batch",
           "lpvmpc_wall_default_config", "lpvmpc_race_walls", "lpvmpc_race_walls_read", "lpvmpc_wall_step_batch",
           "lpvmpc_contact_default_config", "lpvmpc_race_contact", "lpvmpc_race_contact_read", "lpvmpc_contact_step_batch",
           "lpvmpc_event_default_config", "lpvmpc_race_events", "lpvmpc_race_events_read", "lpvmpc_event_step_batch")

_lib = None


def _bind_to_torchs_hip_runtime():
    """A PyTorch-ROCm wheel ships its own HIP / HSA runtime (torch/lib/libamdhip64.so, same SONAME as the system's).  Two HIP
    runtimes cannot both own the GPU in one process: with the system runtime loaded first (by liblpvmpc.so), torch's later
    initialisation reports "No HIP GPUs are available"; with torch's loaded first, liblpvmpc.so binds to it and streams and device
    pointers are shared.  So, where such a wheel is installed and torch is not imported yet, its runtime is loaded here (the
    shared object only -- torch itself is not imported).  LPVMPC_SYSTEM_HIP=1 keeps the system runtime (processes that never use torch)."""
    if "torch" in sys.modules or os.environ.get("LPVMPC_SYSTEM_HIP"):
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        for d in (spec.submodule_search_locations if spec else []):
            cand = os.path.join(d, "lib", "libamdhip64.so")
            if os.path.exists(cand):
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
                return
    except Exception:           # no torch, or an unusual layout: the system runtime it is
        pass


def load():
    """Load liblpvmpc.so; in a process that has (or may later import) a PyTorch-ROCm wheel it binds to that wheel's HIP runtime
    (see _bind_to_torchs_hip_runtime), so the order of `import torch` and the first lpvmpc call does not matter."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s not found -- build it with `python __graft_entry__.py` (or `make -C %s`); "
                          "there is no CPU fallback" % (LIB_PATH, os.path.join(_HERE, "csrc")))
    _bind_to_torchs_hip_runtime()
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL if "torch" in sys.modules else C.RTLD_LOCAL)
    P = C.POINTER
    vp = C.c_void_p
    lib.lpvmpc_version.restype = C.c_int
    lib.lpvmpc_default_config.argtypes = [_i, P(Config)]
    lib.lpvmpc_default_config.restype = None
    lib.lpvmpc_create.argtypes = [P(Config)]
    lib.lpvmpc_create.restype = vp
    lib.lpvmpc_destroy.argtypes = [vp]
    lib.lpvmpc_destroy.restype = None
    lib.lpvmpc_last_error.argtypes = [vp]
    lib.lpvmpc_last_error.restype = C.c_char_p
    lib.lpvmpc_last_error_code.argtypes = []
    lib.lpvmpc_last_error_code.restype = C.c_int
    lib.lpvmpc_reserve.argtypes = [vp, _i]
    lib.lpvmpc_lpv_batch.argtypes = [vp, _i, vp, vp, vp, vp, _d, _i, vp, vp, vp]
    lib.lpvmpc_estimate_abc_batch.argtypes = [vp, _i, vp, vp, vp, vp]
    lib.lpvmpc_solve_batch_AB.argtypes = [vp, _i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.lpvmpc_solve_batch.argtypes = [vp, _i, vp, vp, vp, vp, vp, vp, _d, _i, vp, vp, vp, vp, vp, vp]
    lib.lpvmpc_solve_batch_dev.argtypes = [vp, _i, vp, vp, vp, vp, vp, vp, _d, _i, vp, vp, vp, vp, vp, vp, vp]
    lib.lpvmpc_last_kernel_ms.argtypes = [vp]
    lib.lpvmpc_last_kernel_ms.restype = _d
    lib.lpvmpc_set_timing.argtypes = [vp, _i]
    lib.lpvmpc_set_option.argtypes = [vp, C.c_char_p, _i]
    lib.lpvmpc_set_option.restype = C.c_int
    lib.lpvmpc_kernel_time_stats.argtypes = [vp, P(_d), P(_i)]
    lib.lpvmpc_kernel_time_stats.restype = C.c_int
    lib.lpvmpc_local_position_batch.argtypes = [vp, _i, vp, _d, _d, vp]
    lib.lpvmpc_global_position_batch.argtypes = [vp, _i, vp, vp]
    lib.lpvmpc_plant_step_batch.argtypes = [vp, _i, vp, vp, _i, _d, _d]
    lib.lpvmpc_cl_init.argtypes = [vp, _i, vp, _d, _d, _i, _i, _d, _d]
    lib.lpvmpc_cl_tick.argtypes = [vp, _i]
    lib.lpvmpc_cl_read.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.lpvmpc_cl_release.argtypes = [vp]
    lib.lpvmpc_join.argtypes = [vp, vp]
    lib.lpvmpc_resume_time_stats.argtypes = [vp, P(_d), P(_i)]
    try:        # (tools/ab_equal.py / ab_lib.sh load older builds of the library through this module: round 5's has no such export)
        lib.lpvmpc_defer_stats.argtypes = [vp, P(C.c_int64), P(C.c_int64)]
        lib.lpvmpc_defer_stats.restype = C.c_int
    except AttributeError:
        pass
    lib.lpvmpc_handoff_default_config.argtypes = [P(HandoffConfig)]
    lib.lpvmpc_handoff_default_config.restype = None
    lib.lpvmpc_handoff_length.argtypes = [_i, _d, P(HandoffConfig)]
    lib.lpvmpc_handoff_operators.argtypes = [_i, _d, P(HandoffConfig), vp, vp]
    lib.lpvmpc_handoff_setup.argtypes = [vp, P(HandoffConfig)]
    lib.lpvmpc_handoff_batch.argtypes = [vp, _i, vp, vp, vp, vp, vp]
    lib.lpvmpc_cascade_init.argtypes = [vp, vp, _i, vp, vp, vp, _i, _d, _d, _d, _i, vp, _d, _d]
    lib.lpvmpc_cascade_tick.argtypes = [vp, _i]
    lib.lpvmpc_cascade_read.argtypes = [vp] + [vp] * 12
    lib.lpvmpc_cascade_alive_ticks.argtypes = [vp, vp]
    lib.lpvmpc_cascade_alive_ticks.restype = C.c_int
    lib.lpvmpc_observer_default_config.argtypes = [P(ObserverConfig)]
    lib.lpvmpc_observer_default_config.restype = None
    lib.lpvmpc_observer_setup.argtypes = [vp, P(ObserverConfig)]
    lib.lpvmpc_observer_read.argtypes = [vp, vp, vp]
    lib.lpvmpc_observer_step_batch.argtypes = [vp, _i, P(ObserverConfig), vp, vp, vp, vp, vp]
    for name in ("lpvmpc_observer_setup", "lpvmpc_observer_read", "lpvmpc_observer_step_batch"):
        getattr(lib, name).restype = C.c_int
    try:        # (older builds loaded by tools/ab_equal.py have no race engine)
        lib.lpvmpc_solve_batch_masked.argtypes = [vp, _i, vp, vp, vp, vp, vp, vp, _d, _i, vp, vp, vp, vp, vp, vp, vp]
        lib.lpvmpc_race_default_config.argtypes = [P(RaceConfig)]
        lib.lpvmpc_race_default_config.restype = None
        lib.lpvmpc_race_init.argtypes = [vp, vp, vp, _i, vp, vp, P(RaceConfig)]
        lib.lpvmpc_race_tick.argtypes = [vp, _i]
        lib.lpvmpc_race_read.argtypes = [vp] + [vp] * 10
        lib.lpvmpc_race_laps.argtypes = [vp, vp, vp]
        lib.lpvmpc_race_predictions.argtypes = [vp, vp, vp]
        for name in ("lpvmpc_solve_batch_masked", "lpvmpc_race_init", "lpvmpc_race_tick", "lpvmpc_race_read", "lpvmpc_race_laps",
                     "lpvmpc_race_predictions"):
            getattr(lib, name).restype = C.c_int
    except AttributeError:
        pass
    try:        # (nor the race with an estimator)
        lib.lpvmpc_race_init_observed.argtypes = [vp, vp, vp, _i, vp, vp, P(RaceConfig), P(ObserverConfig)]
        lib.lpvmpc_race_init_observed.restype = C.c_int
    except AttributeError:
        pass
    try:        # (nor the actuator model)
        lib.lpvmpc_actuator_default_config.argtypes = [P(ActuatorConfig)]
        lib.lpvmpc_actuator_default_config.restype = None
        lib.lpvmpc_plant_step_actuated_batch.argtypes = [vp, _i, vp, vp, vp, _i, _d, _d, P(ActuatorConfig), vp, vp]
        lib.lpvmpc_cl_init_actuated.argtypes = [vp, _i, vp, _d, _d, _i, _i, _d, _d, P(ActuatorConfig), vp, vp]
        lib.lpvmpc_race_init_actuated.argtypes = [vp, vp, vp, _i, vp, vp, P(RaceConfig), P(ObserverConfig), P(ActuatorConfig), vp, vp]
        lib.lpvmpc_actuator_read.argtypes = [vp, vp, vp, vp]
        for name in ("lpvmpc_plant_step_actuated_batch", "lpvmpc_cl_init_actuated", "lpvmpc_race_init_actuated", "lpvmpc_actuator_read"):
            getattr(lib, name).restype = C.c_int
    except AttributeError:
        pass
    try:        # (nor the per-vehicle plant parameters)
        lib.lpvmpc_plant_step_vehicles_batch.argtypes = [vp, _i, vp, vp, vp, _i, _d, _d, P(ActuatorConfig), vp, vp, vp]
        lib.lpvmpc_cl_init_vehicles.argtypes = [vp, _i, vp, _d, _d, _i, _i, _d, _d, P(ActuatorConfig), vp, vp, vp]
        lib.lpvmpc_race_init_vehicles.argtypes = [vp, vp, vp, _i, vp, vp, P(RaceConfig), P(ObserverConfig), P(ActuatorConfig), vp, vp, vp]
        lib.lpvmpc_plant_params_read.argtypes = [vp, vp]
        for name in ("lpvmpc_plant_step_vehicles_batch", "lpvmpc_cl_init_vehicles", "lpvmpc_race_init_vehicles", "lpvmpc_plant_params_read"):
            getattr(lib, name).restype = C.c_int
    except AttributeError:
        pass
    try:        # (nor the per-vehicle model parameters)
        lib.lpvmpc_set_model_params.argtypes = [vp, _i, vp]
        lib.lpvmpc_model_params_read.argtypes = [vp, P(_i), vp]
        for name in ("lpvmpc_set_model_params", "lpvmpc_model_params_read"):
            getattr(lib, name).restype = C.c_int
    except AttributeError:
        pass
    try:        # (nor the per-vehicle tunings)
        lib.lpvmpc_set_tunings.argtypes = [vp, _i, vp]
        lib.lpvmpc_tunings_read.argtypes = [vp, P(_i), vp]
        lib.lpvmpc_tuning_from_config.argtypes = [P(Config), vp]
        lib.lpvmpc_tuning_device_row.argtypes = [_i, vp, vp]
        for name in ("lpvmpc_set_tunings", "lpvmpc_tunings_read", "lpvmpc_tuning_from_config", "lpvmpc_tuning_device_row"):
            getattr(lib, name).restype = C.c_int
    except AttributeError:
        pass
    try:        # (nor the tyre model)
        lib.lpvmpc_plant_step_tyres_batch.argtypes = [vp, _i, vp, vp, vp, _i, _d, _d, P(ActuatorConfig), vp, vp, vp, vp]
        lib.lpvmpc_cl_init_tyres.argtypes = [vp, _i, vp, _d, _d, _i, _i, _d, _d, P(ActuatorConfig), vp, vp, vp, vp]
        lib.lpvmpc_race_init_tyres.argtypes = [vp, vp, vp, _i, vp, vp, P(RaceConfig), P(ObserverConfig), P(ActuatorConfig), vp, vp, vp, vp]
        lib.lpvmpc_tyre_params_read.argtypes = [vp, vp]
        lib.lpvmpc_tyre_force_batch.argtypes = [vp, _i, vp, vp, vp, vp]
        for name in ("lpvmpc_plant_step_tyres_batch", "lpvmpc_cl_init_tyres", "lpvmpc_race_init_tyres", "lpvmpc_tyre_params_read",
                     "lpvmpc_tyre_force_batch",
           "lpvmpc_observer_default_design", "lpvmpc_observer_design_batch", "lpvmpc_set_observer_vehicles",
           "lpvmpc_observer_vehicles_read", "lpvmpc_observer_step_vehicles_batch"):
            getattr(lib, name).restype = C.c_int
    except AttributeError:
        pass
    try:        # (nor the estimator's gain design)
        lib.lpvmpc_observer_default_design.argtypes = [P(ObserverDesign)]
        lib.lpvmpc_observer_default_design.restype = None
        lib.lpvmpc_observer_design_batch.argtypes = [vp, _i, vp, P(ObserverDesign), vp, vp, vp]
        lib.lpvmpc_observer_design_batch.restype = C.c_int
        lib.lpvmpc_set_observer_vehicles.argtypes = [vp, _i, vp, vp, vp, P(ObserverDesign)]
        lib.lpvmpc_observer_vehicles_read.argtypes = [vp, P(_i), vp, vp, vp]
        lib.lpvmpc_observer_step_vehicles_batch.argtypes = [vp, _i, P(ObserverConfig), vp, vp, vp, vp, vp, vp, vp, vp]
        for name in ("lpvmpc_set_observer_vehicles", "lpvmpc_observer_vehicles_read", "lpvmpc_observer_step_vehicles_batch"):
            getattr(lib, name).restype = C.c_int
    except AttributeError:
        pass
    try:        # (nor the per-vehicle tracks)
        lib.lpvmpc_set_tracks.argtypes = [vp, _i, vp, vp, vp, vp, _i, vp]
        lib.lpvmpc_tracks_read.argtypes = [vp, P(_i), P(_i), vp, vp, vp, vp, vp]
        for name in ("lpvmpc_set_tracks", "lpvmpc_tracks_read"):
            getattr(lib, name).restype = C.c_int
    except AttributeError:
        pass
    try:        # (nor the plant disturbances)
        lib.lpvmpc_disturbance_default_config.argtypes = [P(DisturbanceConfig)]
        lib.lpvmpc_disturbance_default_config.restype = None
        lib.lpvmpc_set_disturbances.argtypes = [vp, _i, P(DisturbanceConfig), vp]
        lib.lpvmpc_disturbances_read.argtypes = [vp, vp, vp]
        lib.lpvmpc_plant_step_disturbed_batch.argtypes = [vp, _i, vp, vp, vp, _i, _d, _d, P(ActuatorConfig), vp, vp, vp, vp,
                                                          P(DisturbanceConfig), vp, vp]
        for name in ("lpvmpc_set_disturbances", "lpvmpc_disturbances_read", "lpvmpc_plant_step_disturbed_batch"):
            getattr(lib, name).restype = C.c_int
    except AttributeError:
        pass
    try:        # (nor the tyre wear and temperature)
        lib.lpvmpc_set_tyre_wear.argtypes = [vp, _i, vp]
        lib.lpvmpc_tyre_wear_read.argtypes = [vp, vp, vp]
        lib.lpvmpc_tyre_wear_fit.argtypes = [vp, vp]
        lib.lpvmpc_plant_step_worn_batch.argtypes = [vp, _i, vp, vp, vp, _i, _d, _d, P(ActuatorConfig), vp, vp, vp, vp,
                                                     P(DisturbanceConfig), vp, vp, vp, vp]
        for name in ("lpvmpc_set_tyre_wear", "lpvmpc_tyre_wear_read", "lpvmpc_tyre_wear_fit", "lpvmpc_plant_step_worn_batch"):
            getattr(lib, name).restype = C.c_int
    except AttributeError:
        pass
    try:        # (nor the sensor faults)
        lib.lpvmpc_sensor_fault_default_config.argtypes = [P(SensorFaultConfig)]
        lib.lpvmpc_sensor_fault_default_config.restype = None
        lib.lpvmpc_set_sensor_faults.argtypes = [vp, _i, P(SensorFaultConfig), vp]
        lib.lpvmpc_sensor_faults_read.argtypes = [vp, P(_i), vp]
        lib.lpvmpc_sensor_step_batch.argtypes = [vp, _i, P(ObserverConfig), _d, P(SensorFaultConfig), vp, vp, vp, vp, vp]
        for name in ("lpvmpc_set_sensor_faults", "lpvmpc_sensor_faults_read", "lpvmpc_sensor_step_batch"):
            getattr(lib, name).restype = C.c_int
    except AttributeError:
        pass
    try:        # (nor the race recorder)
        lib.lpvmpc_race_record.argtypes = [vp, P(RaceRecordConfig)]
        lib.lpvmpc_race_record_read.argtypes = [vp, _i, vp, vp, vp, vp]
        lib.lpvmpc_race_lap_stats.argtypes = [vp, vp, vp, vp]
        for name in ("lpvmpc_race_record", "lpvmpc_race_record_read", "lpvmpc_race_lap_stats"):
            getattr(lib, name).restype = C.c_int
    except AttributeError:
        pass
    try:        # (nor the race's snapshot, restore and clone)
        lib.lpvmpc_race_snapshot_size.argtypes = [vp, P(C.c_int64)]
        lib.lpvmpc_race_snapshot.argtypes = [vp, vp, C.c_int64]
        lib.lpvmpc_race_restore.argtypes = [vp, vp, C.c_int64]
        lib.lpvmpc_race_clone.argtypes = [vp, vp, P(_i)]
        for name in ("lpvmpc_race_snapshot_size", "lpvmpc_race_snapshot", "lpvmpc_race_restore", "lpvmpc_race_clone"):
            getattr(lib, name).restype = C.c_int
    except AttributeError:
        pass
    try:        # (nor the heats)
        lib.lpvmpc_heats_default_config.argtypes = [P(HeatsConfig)]
        lib.lpvmpc_heats_default_config.restype = None
        lib.lpvmpc_race_heats.argtypes = [vp, P(HeatsConfig), vp, vp]
        lib.lpvmpc_race_standings.argtypes = [vp, vp, vp, vp, vp]
        lib.lpvmpc_heat_step_batch.argtypes = [vp, _i, _i, vp, vp, P(HeatsConfig), _i, vp, vp, vp, vp, vp, vp, vp, vp]
        for name in ("lpvmpc_race_heats", "lpvmpc_race_standings", "lpvmpc_heat_step_batch"):
            getattr(lib, name).restype = C.c_int
    except AttributeError:
        pass
    try:        # (nor the interactions)
        lib.lpvmpc_interaction_default_config.argtypes = [P(InteractionConfig)]
        lib.lpvmpc_interaction_default_config.restype = None
        lib.lpvmpc_race_interactions.argtypes = [vp, P(InteractionConfig)]
        lib.lpvmpc_race_interactions_read.argtypes = [vp, vp, vp]
        lib.lpvmpc_interaction_step_batch.argtypes = [vp, _i, _i, vp, P(HeatsConfig), P(InteractionConfig), _i, vp, vp, vp, vp, vp, vp, vp, vp]
        for name in ("lpvmpc_race_interactions", "lpvmpc_race_interactions_read", "lpvmpc_interaction_step_batch"):
            getattr(lib, name).restype = C.c_int
    except AttributeError:
        pass
    try:        # (nor the walls)
        lib.lpvmpc_wall_default_config.argtypes = [P(WallConfig)]
        lib.lpvmpc_wall_default_config.restype = None
        lib.lpvmpc_race_walls.argtypes = [vp, P(WallConfig)]
        lib.lpvmpc_race_walls_read.argtypes = [vp, vp, vp]
        lib.lpvmpc_wall_step_batch.argtypes = [vp, _i, P(WallConfig), _d, _i, vp, vp, vp, vp, vp, vp, vp]
        for name in ("lpvmpc_race_walls", "lpvmpc_race_walls_read", "lpvmpc_wall_step_batch"):
            getattr(lib, name).restype = C.c_int
    except AttributeError:
        pass
    try:        # (nor the contact model)
        lib.lpvmpc_contact_default_config.argtypes = [P(ContactConfig)]
        lib.lpvmpc_contact_default_config.restype = None
        lib.lpvmpc_race_contact.argtypes = [vp, P(ContactConfig)]
        lib.lpvmpc_race_contact_read.argtypes = [vp, vp, vp]
        lib.lpvmpc_contact_step_batch.argtypes = [vp, _i, _i, vp, P(HeatsConfig), P(InteractionConfig), P(ContactConfig), _i] + [vp] * 12
        for name in ("lpvmpc_race_contact", "lpvmpc_race_contact_read", "lpvmpc_contact_step_batch"):
            getattr(lib, name).restype = C.c_int
    except AttributeError:
        pass
    try:        # (nor the race event log)
        lib.lpvmpc_event_default_config.argtypes = [P(EventConfig)]
        lib.lpvmpc_event_default_config.restype = None
        lib.lpvmpc_race_events.argtypes = [vp, P(EventConfig)]
        lib.lpvmpc_race_events_read.argtypes = [vp, _i, P(C.c_int64), P(_i), vp, vp, vp]
        lib.lpvmpc_event_step_batch.argtypes = [vp, _i, _i, vp, vp, vp, _i, vp, vp, vp, vp, vp, C.c_uint32, vp, vp, P(C.c_int64), _i, vp, vp,
                                                P(_i), vp]
        for name in ("lpvmpc_race_events", "lpvmpc_race_events_read", "lpvmpc_event_step_batch"):
            getattr(lib, name).restype = C.c_int
    except AttributeError:
        pass
    for name in ("lpvmpc_handoff_length", "lpvmpc_handoff_operators", "lpvmpc_handoff_setup", "lpvmpc_handoff_batch",
                 "lpvmpc_cascade_init", "lpvmpc_cascade_tick", "lpvmpc_cascade_read"):
        getattr(lib, name).restype = C.c_int
    for name in ("lpvmpc_local_position_batch", "lpvmpc_global_position_batch", "lpvmpc_plant_step_batch",
                 "lpvmpc_cl_init", "lpvmpc_cl_tick", "lpvmpc_cl_read", "lpvmpc_cl_release", "lpvmpc_join", "lpvmpc_resume_time_stats"):
        getattr(lib, name).restype = C.c_int
    for name in ("lpvmpc_reserve", "lpvmpc_lpv_batch", "lpvmpc_estimate_abc_batch", "lpvmpc_solve_batch_AB",
                 "lpvmpc_solve_batch", "lpvmpc_solve_batch_dev", "lpvmpc_set_timing"):
        getattr(lib, name).restype = C.c_int
    _lib = lib
    return lib


def default_config(kind):
    cfg = Config()
    load().lpvmpc_default_config(kind, C.byref(cfg))
    return cfg


def default_handoff_config():
    cfg = HandoffConfig()
    load().lpvmpc_handoff_default_config(C.byref(cfg))
    return cfg


def default_race_config():
    cfg = RaceConfig()
    load().lpvmpc_race_default_config(C.byref(cfg))
    return cfg


def default_actuator_config():
    cfg = ActuatorConfig()
    load().lpvmpc_actuator_default_config(C.byref(cfg))
    return cfg


def default_observer_config():
    cfg = ObserverConfig()
    load().lpvmpc_observer_default_config(C.byref(cfg))
    return cfg


def default_disturbance_config():
    cfg = DisturbanceConfig()
    load().lpvmpc_disturbance_default_config(C.byref(cfg))
    return cfg


def default_sensor_fault_config():
    cfg = SensorFaultConfig()
    load().lpvmpc_sensor_fault_default_config(C.byref(cfg))
    return cfg


def default_interaction_config():
    cfg = InteractionConfig()
    load().lpvmpc_interaction_default_config(C.byref(cfg))
    return cfg


def default_wall_config():
    cfg = WallConfig()
    load().lpvmpc_wall_default_config(C.byref(cfg))
    return cfg


def default_contact_config():
    cfg = ContactConfig()
    load().lpvmpc_contact_default_config(C.byref(cfg))
    return cfg


def default_event_config():
    cfg = EventConfig()
    load().lpvmpc_event_default_config(C.byref(cfg))
    return cfg


def default_observer_design():
    d = ObserverDesign()
    load().lpvmpc_observer_default_design(C.byref(d))
    return d


def f64(a, shape=None, name="array"):
    """Contiguous float64 copy/view with an optional exact shape check."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError("%s has shape %s, expected %s" % (name, a.shape, tuple(shape)))
    return a


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def check(handle, rc):
    if rc != 0:
        msg = load().lpvmpc_last_error(handle)
        raise LpvMpcError(rc, msg.decode() if msg else "?")
