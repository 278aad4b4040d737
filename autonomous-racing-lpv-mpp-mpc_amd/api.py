"""Host-side mirror of the reference's operator interface for the solve path.

* ``PathFollowingLPV_MPC`` / ``LPV_MPC_Planner`` -- drop-ins with the reference's constructor, ``solve``
  and ``LPVPrediction`` signatures and result attributes (reference ControllerObject/PathFollowingLPVMPC.py:30-258,
  PlannerObject/LPV_MPC_Planner.py:29-320), each backed by a batch-of-one call into liblpvmpc.so.
* ``BatchedSolver`` -- the explicit batched interface (thousands of independent instances per launch).

All numerics run in the HIP library; this file only marshals numpy arrays.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import datetime

import numpy as np

from . import _ffi
from ._ffi import KIND_CONTROLLER, KIND_PLANNER, LpvMpcError, STATUS_TEXT, f64, ptr

# MAIN_LAUNCH.launch:5-11,40-41 -- used when neither rospy nor an explicit ``params`` dict is available
DEFAULT_PARAMS = dict(lf=0.125, lr=0.125, m=1.98, Iz=0.03, Cf=60.0, Cr=60.0, mu=0.05, max_vel=5.0, min_vel=0.9)
_ROS_NAMES = dict(lf="lf", lr="lr", m="m", Iz="Iz", Cf="Cf", Cr="Cr", mu="mu",
                  max_vel="/TrajectoryPlanner/max_vel", min_vel="/TrajectoryPlanner/min_vel")


def _vehicle_params(params, need_min_vel):
    """Parameters from an explicit dict, else from the ROS parameter server (CTRL:38-48 / PLAN:70-82),
    else the launch-file defaults."""
    out = dict(DEFAULT_PARAMS)
    if params is not None:
        out.update(params)
        return out
    try:
        import rospy  # noqa: F401  (only present on a ROS box)
    except ImportError:
        return out
    for key, ros_name in _ROS_NAMES.items():
        if key == "min_vel" and not need_min_vel:
            continue
        out[key] = rospy.get_param(ros_name)
    return out


def build_config(kind, N, dt, Q, R, dR, L_cf=None, track=None, params=None, device=0, **settings):
    """The lpvmpc_config of BatchedSolver(kind, N, dt, Q, R, dR, ...) -- same arguments -- without creating a handle (host only)."""
    kind = {"controller": KIND_CONTROLLER, "planner": KIND_PLANNER}.get(kind, kind)
    if kind not in (KIND_CONTROLLER, KIND_PLANNER):
        raise ValueError("kind must be 'controller' or 'planner'")
    nx = 6 if kind == KIND_CONTROLLER else 5
    cfg = _ffi.default_config(kind)
    cfg.N = int(N)
    cfg.device = int(device)
    cfg.dt = float(dt)
    p = dict(DEFAULT_PARAMS)
    if params:
        p.update(params)
    for k in ("lf", "lr", "m", "Iz", "Cf", "Cr", "mu", "max_vel", "min_vel"):
        setattr(cfg, k, float(p[k]))
    Q = f64(Q, (nx, nx), "Q")
    R = f64(R, (2, 2), "R")
    dR = f64(dR, (2,), "dR")
    for i in range(36):
        cfg.Q[i] = 0.0
    for i, v in enumerate(Q.reshape(-1)):
        cfg.Q[i] = v
    for i, v in enumerate(R.reshape(-1)):
        cfg.R[i] = v
    cfg.dR[0], cfg.dR[1] = dR
    for i in range(6):
        cfg.L_cf[i] = 0.0
    if kind == KIND_PLANNER:
        if L_cf is None:
            raise ValueError("the planner needs L_cf")
        for i, v in enumerate(f64(L_cf, (5,), "L_cf")):
            cfg.L_cf[i] = v
    for k, v in settings.items():
        if k not in _ffi.SETTING_FIELDS:
            raise TypeError("unknown setting %r" % k)
        if k.startswith("plan_"):
            arr = getattr(cfg, k)
            for i, x in enumerate(f64(v, (len(arr),), k)):
                arr[i] = x
        else:
            setattr(cfg, k, v)
    if track is not None:
        tab = f64(track, name="track")
        if tab.ndim != 2 or tab.shape[1] != 6 or tab.shape[0] > _ffi.MAX_TRACK_ROWS:
            raise ValueError("track table must be (rows<=%d, 6)" % _ffi.MAX_TRACK_ROWS)
        cfg.track_rows = tab.shape[0]
        for i, v in enumerate(tab.reshape(-1)):
            cfg.track[i] = v
    return cfg


class BatchedSolver:
    """Batched LPV-MPC (``kind="controller"``) / LPV-MPP (``kind="planner"``) solver on one MI355X.

    Parameters follow the reference constructors; ``track`` is a PointAndTangent table (or None when only
    caller-supplied curvature / LPV matrices are used); ``settings`` overrides OSQP settings, the
    controller limits and the planner's boxes (see ``_ffi.SETTING_FIELDS``; ``plan_xmin`` / ``plan_xmax``
    take 5 values, ``plan_umin`` / ``plan_umax`` 2, slots 0 and 3 of the state box are always set from
    min_vel / max_vel and max_ey)."""

    def __init__(self, kind, N, dt, Q, R, dR, L_cf=None, track=None, params=None, device=0, **settings):
        cfg = build_config(kind, N, dt, Q, R, dR, L_cf=L_cf, track=track, params=params, device=device, **settings)
        self.kind = cfg.kind
        self.nx = 6 if self.kind == KIND_CONTROLLER else 5
        self.nu = 2
        self.N = int(N)
        lib = _ffi.load()
        self.cfg = cfg
        self._lib = lib
        self._h = lib.lpvmpc_create(C.byref(cfg))
        if not self._h:
            msg = lib.lpvmpc_last_error(None)
            raise LpvMpcError(lib.lpvmpc_last_error_code() or _ffi.E_ARG, msg.decode() if msg else "lpvmpc_create failed")
        self._ho_M = 0                       # samples per My_Planning array once handoff_setup() has run
        self._cas = self._cas_planner = None
        self._race = None                    # (B, laps, tt, planner) while this engine owns a race
        self._rec = None                     # (capacity, stride) while the race records

    # -- lifetime --------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.lpvmpc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        _ffi.check(self._h, rc)

    def reserve(self, B):
        self._chk(self._lib.lpvmpc_reserve(self._h, int(B)))

    def set_option(self, name, value):
        self._chk(self._lib.lpvmpc_set_option(self._h, name.encode(), int(value)))

    def set_timing(self, on=True):
        self._chk(self._lib.lpvmpc_set_timing(self._h, 1 if on else 0))

    def last_kernel_ms(self):
        return float(self._lib.lpvmpc_last_kernel_ms(self._h))

    def join(self, stream=0):
        """Order ``stream`` behind the outstanding resume launches of the straggler deferral (option "defer_after"): the
        outputs of the deferred calls are complete for work enqueued on ``stream`` afterwards."""
        self._chk(self._lib.lpvmpc_join(self._h, C.c_void_p(int(stream))))

    def defer_stats(self):
        """(parked, refused) of the straggler deferral since the handle's first deferred call (lpvmpc_defer_stats: waits for the
        stream of the last deferred call)."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.lpvmpc_defer_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def resume_time_stats(self):
        tot = C.c_double(0.0); n = C.c_int32(0)
        self._chk(self._lib.lpvmpc_resume_time_stats(self._h, C.byref(tot), C.byref(n)))
        return tot.value, n.value

    def kernel_time_stats(self):
        """(total_ms, launches) of the solve kernel since set_timing(True)."""
        tot, n = C.c_double(0.0), C.c_int32(0)
        self._chk(self._lib.lpvmpc_kernel_time_stats(self._h, C.byref(tot), C.byref(n)))
        return tot.value, n.value

    # -- host-array entry points ------------------------------------------------------------------
    def lpv(self, x0, u_prev, vel_ref=None, curv_s=None, cf_new=60.0, lap=1):
        """Batched LPVPrediction.  Returns (states [B,N,nx], A [B,N,nx,nx], Bm [B,N,nx,2])."""
        N, nx = self.N, self.nx
        x0 = f64(x0).reshape(-1, nx)
        B = x0.shape[0]
        u_prev = f64(u_prev, (B, N, 2), "u_prev")
        ctrl = self.kind == KIND_CONTROLLER
        vel_ref = f64(vel_ref, (B, N + 1), "vel_ref") if ctrl else None
        if curv_s is not None:
            curv_s = f64(curv_s, (B, N) if ctrl else (B, N + 1), "curv_ref" if ctrl else "SS")
        states = np.empty((B, N, nx)); A = np.empty((B, N, nx, nx)); Bm = np.empty((B, N, nx, 2))
        self._chk(self._lib.lpvmpc_lpv_batch(self._h, B, ptr(x0), ptr(u_prev), ptr(vel_ref), ptr(curv_s),
                                             float(cf_new), int(lap), ptr(states), ptr(A), ptr(Bm)))
        return states, A, Bm

    def estimate_abc(self, xlast, delta):
        """Batched _EstimateABC.  xlast [B,N,6], delta [B,N] -> (A, Bm)."""
        N, nx = self.N, self.nx
        xlast = f64(xlast)
        B = xlast.shape[0]
        xlast = f64(xlast, (B, N, 6), "xlast")
        delta = f64(delta, (B, N), "delta")
        A = np.empty((B, N, nx, nx)); Bm = np.empty((B, N, nx, 2))
        self._chk(self._lib.lpvmpc_estimate_abc_batch(self._h, B, ptr(xlast), ptr(delta), ptr(A), ptr(Bm)))
        return A, Bm

    def _outputs(self, B):
        N, nx = self.N, self.nx
        return dict(xPred=np.empty((B, N + 1, nx)), uPred=np.empty((B, N, 2)), status=np.empty(B, np.int32),
                    iters=np.empty(B, np.int32), resid=np.empty((B, 4)), polish=np.empty(B, np.int32))

    def solve_AB(self, x0, A, Bm, vel_ref=None, u_old=None, max_ey=None):
        """QP build + ADMM solve with caller-supplied LPV matrices.  Returns a dict of arrays
        xPred [B,N+1,nx], uPred [B,N,2], status, iters, resid [B,4]=(pri,dua,obj,rho), polish."""
        N, nx = self.N, self.nx
        x0 = f64(x0).reshape(-1, nx)
        B = x0.shape[0]
        A = f64(A, (B, N, nx, nx), "A"); Bm = f64(Bm, (B, N, nx, 2), "B")
        ctrl = self.kind == KIND_CONTROLLER
        vel_ref = f64(vel_ref, (B, N + 1), "vel_ref") if ctrl else None
        u_old = None if u_old is None else f64(u_old, (B, 2 + self.cfg.steering_delay), "u_old")
        max_ey = None if ctrl else f64(np.broadcast_to(np.asarray(max_ey, float), (B,)), (B,), "max_ey")
        o = self._outputs(B)
        self._chk(self._lib.lpvmpc_solve_batch_AB(self._h, B, ptr(x0), ptr(A), ptr(Bm), ptr(vel_ref), ptr(u_old),
                                                  ptr(max_ey), ptr(o["xPred"]), ptr(o["uPred"]), ptr(o["status"]),
                                                  ptr(o["iters"]), ptr(o["resid"]), ptr(o["polish"])))
        return o

    def solve(self, x0, u_prev, vel_ref=None, curv_s=None, u_old=None, max_ey=None, cf_new=60.0, lap=1):
        """Fused tick: LPV evaluation + roll-out, QP build, ADMM solve (host arrays in/out)."""
        N, nx = self.N, self.nx
        x0 = f64(x0).reshape(-1, nx)
        B = x0.shape[0]
        u_prev = f64(u_prev, (B, N, 2), "u_prev")
        ctrl = self.kind == KIND_CONTROLLER
        vel_ref = f64(vel_ref, (B, N + 1), "vel_ref") if ctrl else None
        if curv_s is not None:
            curv_s = f64(curv_s, (B, N) if ctrl else (B, N + 1), "curv_ref" if ctrl else "SS")
        u_old = None if u_old is None else f64(u_old, (B, 2 + self.cfg.steering_delay), "u_old")
        max_ey = None if ctrl else f64(np.broadcast_to(np.asarray(max_ey, float), (B,)), (B,), "max_ey")
        o = self._outputs(B)
        self._chk(self._lib.lpvmpc_solve_batch(self._h, B, ptr(x0), ptr(u_prev), ptr(vel_ref), ptr(curv_s), ptr(u_old),
                                               ptr(max_ey), float(cf_new), int(lap), ptr(o["xPred"]), ptr(o["uPred"]),
                                               ptr(o["status"]), ptr(o["iters"]), ptr(o["resid"]), ptr(o["polish"])))
        return o

    def solve_batch_masked(self, active, x0, u_prev, vel_ref=None, curv_s=None, u_old=None, max_ey=None, cf_new=60.0, lap=1, out=None):
        """``solve`` for the instances with ``active[i] != 0`` only.  The others are not solved and their rows of ``out`` (a dict
        as ``solve`` returns; fresh arrays of zeros when None) are left as they are.  Returns ``out``."""
        N, nx = self.N, self.nx
        x0 = f64(x0).reshape(-1, nx)
        B = x0.shape[0]
        act = np.ascontiguousarray(active, np.int32)
        if act.shape != (B,):
            raise ValueError("active must have shape (%d,)" % B)
        u_prev = f64(u_prev, (B, N, 2), "u_prev")
        ctrl = self.kind == KIND_CONTROLLER
        vel_ref = f64(vel_ref, (B, N + 1), "vel_ref") if ctrl else None
        if curv_s is not None:
            curv_s = f64(curv_s, (B, N) if ctrl else (B, N + 1), "curv_ref" if ctrl else "SS")
        u_old = None if u_old is None else f64(u_old, (B, 2 + self.cfg.steering_delay), "u_old")
        max_ey = None if ctrl else f64(np.broadcast_to(np.asarray(max_ey, float), (B,)), (B,), "max_ey")
        if out is None:
            out = {k: np.zeros_like(v) for k, v in self._outputs(B).items()}
        for k, v in self._outputs(B).items():
            a = out[k]
            if not (isinstance(a, np.ndarray) and a.shape == v.shape and a.dtype == v.dtype and a.flags.c_contiguous):
                raise ValueError("out[%r] must be a C-contiguous %s array of shape %s" % (k, v.dtype, v.shape))
        self._chk(self._lib.lpvmpc_solve_batch_masked(self._h, B, ptr(x0), ptr(u_prev), ptr(vel_ref), ptr(curv_s), ptr(u_old),
                                                      ptr(max_ey), float(cf_new), int(lap), ptr(out["xPred"]), ptr(out["uPred"]),
                                                      ptr(out["status"]), ptr(out["iters"]), ptr(out["resid"]), ptr(out["polish"]), ptr(act)))
        return out

    # -- caller-side helpers and the closed-loop fleet ------------------------------------
    def local_position(self, xy_psi, half_width, slack):
        """Batched Map.getLocalPosition: [B,3] -> [B,4] = (s, ey, epsi, inside)."""
        a = f64(xy_psi).reshape(-1, 3); out = np.empty((a.shape[0], 4))
        self._chk(self._lib.lpvmpc_local_position_batch(self._h, a.shape[0], ptr(a), float(half_width), float(slack), ptr(out)))
        return out

    def global_position(self, s_ey):
        """Batched Map.getGlobalPosition: [B,2] -> [B,3] = (x, y, theta)."""
        a = f64(s_ey).reshape(-1, 2); out = np.empty((a.shape[0], 3))
        self._chk(self._lib.lpvmpc_global_position_batch(self._h, a.shape[0], ptr(a), ptr(out)))
        return out

    def plant_step(self, state, u, n_sub=1, dt_sim=0.005, mu_sim=0.05):
        """n_sub steps of Simulator.f on state [B,8] under u [B,2] = (a, delta); returns the new state."""
        st = f64(state).reshape(-1, 8).copy(); u = f64(u, (st.shape[0], 2), "u")
        self._chk(self._lib.lpvmpc_plant_step_batch(self._h, st.shape[0], ptr(st), ptr(u), int(n_sub), float(dt_sim), float(mu_sim)))
        return st

    def plant_step_actuated(self, state, act_state, u, n_sub=1, dt_sim=0.005, mu_sim=0.05, actuator=None, delay_a=None, delay_df=None):
        """n_sub steps of Simulator.f through the actuator stage (vehicleSimulator.py:53-78) under the held command u [B,2] =
        (motor, servo).  act_state [B, ACT_WORDS] (None: fresh, all zeros) carries the command ring, servo_inp and the step
        counter between calls.  ``actuator``: an ``actuator.actuator_config`` result (None: all off); delay_a / delay_df [B]
        per-vehicle delays in steps (None: the config's).  Returns (state, act_state)."""
        st = f64(state).reshape(-1, 8).copy(); B = st.shape[0]
        u = f64(u, (B, 2), "u")
        act = np.zeros((B, _ffi.ACT_WORDS)) if act_state is None else f64(act_state, (B, _ffi.ACT_WORDS), "act_state").copy()
        cfg = _ffi.default_actuator_config() if actuator is None else actuator
        la, ld = _delay_array(delay_a, B, "delay_a"), _delay_array(delay_df, B, "delay_df")
        self._chk(self._lib.lpvmpc_plant_step_actuated_batch(self._h, B, ptr(st), ptr(act), ptr(u), int(n_sub), float(dt_sim), float(mu_sim),
                                                             C.byref(cfg), ptr(la), ptr(ld)))
        return st, act

    def plant_step_vehicles(self, state, u, plant_params=None, act_state=None, n_sub=1, dt_sim=0.005, mu_sim=0.05, actuator=None,
                            delay_a=None, delay_df=None, tyre_params=None):
        """plant_step_actuated with each vehicle's own plant row: plant_params [B, 7] = (lf, lr, m, Iz, Cf, Cr, mu) per vehicle
        (None: the nominal row of this engine, plant.plant_params; mu_sim is ignored when rows are given).  ``tyre_params`` [B, 4] =
        (kind, B, C, c_f) per vehicle, "pacejka" (the launch file's tyre for every vehicle) or "linear" (kind 0 for every vehicle),
        selects lpvmpc_plant_step_tyres_batch: kind 1 vehicles step with Simulator.pacejka on both axles.  Returns (state, act_state)."""
        st = f64(state).reshape(-1, 8).copy(); B = st.shape[0]
        u = f64(u, (B, 2), "u")
        rows = _plant_rows(plant_params, B)
        act = np.zeros((B, _ffi.ACT_WORDS)) if act_state is None else f64(act_state, (B, _ffi.ACT_WORDS), "act_state").copy()
        cfg = _ffi.default_actuator_config() if actuator is None else _actuator_cfg(actuator)
        la, ld = _delay_array(delay_a, B, "delay_a"), _delay_array(delay_df, B, "delay_df")
        if tyre_params is not None:
            self._chk(self._lib.lpvmpc_plant_step_tyres_batch(self._h, B, ptr(st), ptr(act), ptr(u), int(n_sub), float(dt_sim), float(mu_sim),
                                                              C.byref(cfg), ptr(la), ptr(ld), ptr(rows), ptr(_tyre_rows(tyre_params, B))))
            return st, act
        self._chk(self._lib.lpvmpc_plant_step_vehicles_batch(self._h, B, ptr(st), ptr(act), ptr(u), int(n_sub), float(dt_sim), float(mu_sim),
                                                             C.byref(cfg), ptr(la), ptr(ld), ptr(rows)))
        return st, act

    def plant_step_disturbed(self, state, u, rows, dist_state=None, seed=0, vehicle_offset=0, n_bound=None, plant_params=None,
                             tyre_params=None, act_state=None, n_sub=1, dt_sim=0.005, mu_sim=0.05, actuator=None, delay_a=None,
                             delay_df=None):
        """plant_step_vehicles as one control tick of n_sub steps with the plant disturbances in front of it
        (lpvmpc_plant_step_disturbed_batch): ``rows`` [B, 13] (disturbance.disturbance_rows), ``dist_state`` [B, 5] = (d_ax, d_ay,
        d_aw, ticks, gamma) carried between calls (None: fresh).  The grip patches are placed on this engine's track, or on its
        track binding.  Returns (state, act_state, dist_state)."""
        from .disturbance import check_disturbance_rows, disturbance_config
        st = f64(state).reshape(-1, 8).copy(); B = st.shape[0]
        u = f64(u, (B, 2), "u")
        prow = _plant_rows(plant_params, B)
        act = np.zeros((B, _ffi.ACT_WORDS)) if act_state is None else f64(act_state, (B, _ffi.ACT_WORDS), "act_state").copy()
        ds = np.zeros((B, _ffi.DIST_STATE)) if dist_state is None else f64(dist_state, (B, _ffi.DIST_STATE), "dist_state").copy()
        if dist_state is None:
            ds[:, 4] = 1.0
        cfg = _ffi.default_actuator_config() if actuator is None else _actuator_cfg(actuator)
        la, ld = _delay_array(delay_a, B, "delay_a"), _delay_array(delay_df, B, "delay_df")
        dc = disturbance_config(seed, vehicle_offset, n_bound)
        r = check_disturbance_rows(rows, B)
        self._chk(self._lib.lpvmpc_plant_step_disturbed_batch(self._h, B, ptr(st), ptr(act), ptr(u), int(n_sub), float(dt_sim), float(mu_sim),
                                                              C.byref(cfg), ptr(la), ptr(ld), ptr(prow),
                                                              ptr(None if tyre_params is None else _tyre_rows(tyre_params, B)),
                                                              C.byref(dc), ptr(r), ptr(ds)))
        return st, act, ds

    def set_disturbances(self, rows, seed=0, vehicle_offset=0, n_bound=None):
        """Attach plant disturbances to the lap-0 fleet or race this engine runs (lpvmpc_set_disturbances; the path engine, for a
        race), from the next tick on: ``rows`` [B, 13] (disturbance.disturbance_rows / sample_disturbances).  The fleet or race must
        have been started with ``tyre_params`` ("linear": kind 0 rows).  ``None`` detaches and restores the base plant / tyre rows."""
        from .disturbance import check_disturbance_rows, disturbance_config
        race = getattr(self, "_race", None) is not None
        B = self._race[0] if race else getattr(self, "_cl_B", 0)
        if rows is None:
            self._chk(self._lib.lpvmpc_set_disturbances(self._h, B, None, None))
            return
        r = check_disturbance_rows(rows, np.asarray(rows).shape[0] if np.asarray(rows).ndim == 2 else B)
        dc = disturbance_config(seed, vehicle_offset, n_bound)
        self._chk(self._lib.lpvmpc_set_disturbances(self._h, r.shape[0], C.byref(dc), ptr(r)))

    def disturbances_read(self):
        """The attached rows [B, 13] and the model's state [B, 5] = (d_ax, d_ay, d_aw, ticks, gamma) (lpvmpc_disturbances_read)."""
        race = getattr(self, "_race", None) is not None
        B = self._race[0] if race else getattr(self, "_cl_B", 0)
        rows, state = np.empty((B, _ffi.DIST_WORDS)), np.empty((B, _ffi.DIST_STATE))
        self._chk(self._lib.lpvmpc_disturbances_read(self._h, ptr(rows), ptr(state)))
        return rows, state

    def plant_step_worn(self, state, u, wear_rows, wear_state=None, rows=None, dist_state=None, seed=0, vehicle_offset=0, n_bound=None,
                        plant_params=None, tyre_params=None, act_state=None, n_sub=1, dt_sim=0.005, mu_sim=0.05, actuator=None,
                        delay_a=None, delay_df=None):
        """plant_step_disturbed with the tyre wear and temperature model behind the disturbances' and in front of the n_sub steps
        (lpvmpc_plant_step_worn_batch): ``wear_rows`` [B, 12] (tyre_wear.tyre_wear_rows), ``wear_state`` [B, 6] = (W, T, P, g, ticks,
        E) carried between calls (None: fresh); ``rows`` None: no disturbance model.  Returns (state, act_state, dist_state,
        wear_state), dist_state None without disturbance rows."""
        from .disturbance import check_disturbance_rows, disturbance_config
        from .tyre_wear import check_tyre_wear_rows
        st = f64(state).reshape(-1, 8).copy(); B = st.shape[0]
        u = f64(u, (B, 2), "u")
        prow = _plant_rows(plant_params, B)
        act = np.zeros((B, _ffi.ACT_WORDS)) if act_state is None else f64(act_state, (B, _ffi.ACT_WORDS), "act_state").copy()
        wr = check_tyre_wear_rows(wear_rows, B)
        ws = np.zeros((B, _ffi.WEAR_STATE)) if wear_state is None else f64(wear_state, (B, _ffi.WEAR_STATE), "wear_state").copy()
        if wear_state is None:
            ws[:, 1] = wr[:, 11]; ws[:, 3] = 1.0
        ds = r = None
        if rows is not None:
            r = check_disturbance_rows(rows, B)
            ds = np.zeros((B, _ffi.DIST_STATE)) if dist_state is None else f64(dist_state, (B, _ffi.DIST_STATE), "dist_state").copy()
            if dist_state is None:
                ds[:, 4] = 1.0
        cfg = _ffi.default_actuator_config() if actuator is None else _actuator_cfg(actuator)
        la, ld = _delay_array(delay_a, B, "delay_a"), _delay_array(delay_df, B, "delay_df")
        dc = disturbance_config(seed, vehicle_offset, n_bound)
        self._chk(self._lib.lpvmpc_plant_step_worn_batch(self._h, B, ptr(st), ptr(act), ptr(u), int(n_sub), float(dt_sim), float(mu_sim),
                                                         C.byref(cfg), ptr(la), ptr(ld), ptr(prow),
                                                         ptr(None if tyre_params is None else _tyre_rows(tyre_params, B)),
                                                         C.byref(dc), ptr(r), ptr(ds), ptr(wr), ptr(ws)))
        return st, act, ds, ws

    def _fleet_B(self):
        return self._race[0] if getattr(self, "_race", None) is not None else getattr(self, "_cl_B", 0)

    def set_tyre_wear(self, rows):
        """Attach tyre wear and temperature to the lap-0 fleet or race this engine runs (lpvmpc_set_tyre_wear; the path engine, for a
        race), from the next tick on: ``rows`` [B, 12] (tyre_wear.tyre_wear_rows / sample_tyre_wear).  The fleet or race must have
        been started with ``tyre_params`` ("linear": kind 0 rows).  ``None`` detaches: the live words go back to the disturbances'
        gamma * base, or to the base rows."""
        from .tyre_wear import check_tyre_wear_rows
        B = self._fleet_B()
        if rows is None:
            self._chk(self._lib.lpvmpc_set_tyre_wear(self._h, B, None))
            return
        r = check_tyre_wear_rows(rows, np.asarray(rows).shape[0] if np.asarray(rows).ndim == 2 else B)
        self._chk(self._lib.lpvmpc_set_tyre_wear(self._h, r.shape[0], ptr(r)))

    def tyre_wear_read(self):
        """The attached rows [B, 12] and the tyre sets' state [B, 6] = (W, T, P, g, ticks, E) (lpvmpc_tyre_wear_read)."""
        B = self._fleet_B()
        rows, state = np.empty((B, _ffi.WEAR_WORDS)), np.empty((B, _ffi.WEAR_STATE))
        self._chk(self._lib.lpvmpc_tyre_wear_read(self._h, ptr(rows), ptr(state)))
        return rows, state

    def tyre_wear_fit(self, mask):
        """A tyre change between ticks (lpvmpc_tyre_wear_fit): the vehicles of ``mask`` [B] start a fresh set (W 0, T_start, P 0, g 1)
        and keep their tick count and energy."""
        m = np.ascontiguousarray(np.asarray(mask).astype(bool).astype(np.int32))
        if m.shape != (self._fleet_B(),):
            raise ValueError("tyre_wear_fit: mask has shape %s, expected (%d,)" % (m.shape, self._fleet_B()))
        self._chk(self._lib.lpvmpc_tyre_wear_fit(self._h, ptr(m)))

    def set_sensor_faults(self, rows, seed=0, vehicle_offset=0):
        """Attach sensor faults to the lap-0 fleet or race this engine runs (lpvmpc_set_sensor_faults; the path engine, for a race),
        from the next tick on: ``rows`` [B, 12] (sensor_faults.fault_rows / sample_faults).  The fleet or race must have the estimator
        in the loop and have been started with ``tyre_params`` ("linear": kind 0 rows).  ``None`` detaches."""
        from .sensor_faults import check_fault_rows, sensor_fault_config
        race = getattr(self, "_race", None) is not None
        B = self._race[0] if race else getattr(self, "_cl_B", 0)
        if rows is None:
            self._chk(self._lib.lpvmpc_set_sensor_faults(self._h, B, None, None))
            return
        r = check_fault_rows(rows, np.asarray(rows).shape[0] if np.asarray(rows).ndim == 2 else B)
        fc = sensor_fault_config(seed, vehicle_offset)
        self._chk(self._lib.lpvmpc_set_sensor_faults(self._h, r.shape[0], C.byref(fc), ptr(r)))

    def sensor_faults(self):
        """The attached sensor fault rows [B, 12], or None with none attached (lpvmpc_sensor_faults_read)."""
        n = C.c_int32(0)
        self._chk(self._lib.lpvmpc_sensor_faults_read(self._h, C.byref(n), None))
        if n.value == 0:
            return None
        rows = np.empty((n.value, _ffi.FAULT_WORDS))
        self._chk(self._lib.lpvmpc_sensor_faults_read(self._h, C.byref(n), ptr(rows)))
        return rows

    def sensor_step(self, cfg, obs_state, plant, servo, motor, rows=None, seed=0, vehicle_offset=0, dt_sim=0.005):
        """One sensors + observer sub-step per vehicle on caller arrays (lpvmpc_sensor_step_batch), as the fused fleet kernels run it
        once per plant step: ``obs_state`` [B, 18] (sensor_faults.OBS_STATE_NAMES), ``plant`` [B, 8] the plant state just advanced,
        ``servo`` / ``motor`` [B] the commanded input, ``cfg`` the estimator configuration.  ``rows`` [B, 12]: the faulted sensor stage
        (None: the healthy one).  An engine with per-vehicle estimator rows bound runs the bound form.  Returns the new state."""
        from .sensor_faults import check_fault_rows, sensor_fault_config
        os_ = f64(obs_state).reshape(-1, _ffi.OBS_STATE_WORDS).copy()
        B = os_.shape[0]
        p = f64(plant, (B, 8), "plant")
        sv = np.ascontiguousarray(np.broadcast_to(np.asarray(servo, float), (B,)))
        mo = np.ascontiguousarray(np.broadcast_to(np.asarray(motor, float), (B,)))
        r = None if rows is None else check_fault_rows(rows, B)
        fc = sensor_fault_config(seed, vehicle_offset)
        self._chk(self._lib.lpvmpc_sensor_step_batch(self._h, B, C.byref(cfg), float(dt_sim), C.byref(fc), ptr(r), ptr(os_), ptr(p), ptr(sv),
                                                     ptr(mo)))
        return os_

    def tyre_force(self, tyre_params, m, alpha):
        """The tyre curve on the device (lpvmpc_tyre_force_batch): force [B] of tyre row b at slip angle alpha [B] for mass m
        (scalar or [B]); tyre_params [B, 4] or "pacejka"."""
        al = f64(alpha).reshape(-1); B = al.shape[0]
        mm = np.ascontiguousarray(np.broadcast_to(np.asarray(m, np.float64), (B,)))
        out = np.empty(B)
        self._chk(self._lib.lpvmpc_tyre_force_batch(self._h, B, ptr(_tyre_rows(tyre_params, B)), ptr(mm), ptr(al), ptr(out)))
        return out

    def tyre_params_read(self):
        """The tyre rows [B, 4] of the fleet / race this engine runs, started with ``tyre_params`` (lpvmpc_tyre_params_read)."""
        race = getattr(self, "_race", None) is not None
        B = self._race[0] if race else getattr(self, "_cl_B", 0)
        out = np.empty((B, _ffi.TYRE_WORDS))
        self._chk(self._lib.lpvmpc_tyre_params_read(self._h, ptr(out)))
        return out

    def plant_params_read(self):
        """The plant rows [B, 7] of the fleet / race this engine runs, started with ``plant_params`` (lpvmpc_plant_params_read)."""
        race = getattr(self, "_race", None) is not None
        B = self._race[0] if race else getattr(self, "_cl_B", 0)
        out = np.empty((B, _ffi.PLANT_WORDS))
        self._chk(self._lib.lpvmpc_plant_params_read(self._h, ptr(out)))
        return out

    def set_model_params(self, rows):
        """Bind per-vehicle model rows [B, 7] = (lf, lr, m, Iz, Cf, Cr, mu) to this engine (lpvmpc_set_model_params): every call
        that linearises -- lpv, estimate_abc, solve*, and a fleet, cascade or race started afterwards -- then takes vehicle b's row
        instead of the engine's own vehicle, must have batch size B, and in the controller roll-out takes the row's Cf for both
        axles (cf_new is ignored).  ``None`` unbinds.  Refused while the engine runs a fleet, cascade or race."""
        if rows is None:
            self._chk(self._lib.lpvmpc_set_model_params(self._h, 0, None))
            return
        a = np.asarray(rows)
        if a.ndim != 2 or a.shape[0] < 1:
            raise ValueError("model_params has shape %s, expected (B, %d) with B >= 1" % (a.shape, _ffi.MODEL_WORDS))
        from .model import check_model_params
        a = check_model_params(a, a.shape[0])
        self._chk(self._lib.lpvmpc_set_model_params(self._h, a.shape[0], ptr(a)))

    def model_params_read(self):
        """The bound model rows [B, 7] (lpvmpc_model_params_read), or None while nothing is bound."""
        B = C.c_int32(0)
        self._chk(self._lib.lpvmpc_model_params_read(self._h, C.byref(B), None))
        if B.value == 0:
            return None
        out = np.empty((B.value, _ffi.MODEL_WORDS))
        self._chk(self._lib.lpvmpc_model_params_read(self._h, C.byref(B), ptr(out)))
        return out

    def set_tracks(self, maps, track_of):
        """Bind per-vehicle tracks to this engine (lpvmpc_set_tracks): ``maps`` is a sequence (the palette, at most 64) of objects with
        ``.PointAndTangent``, ``.halfWidth`` and ``.slack`` -- ``track.Map``, ``track.mirrored`` / ``track.scaled`` results, the
        reference's own Map -- and ``track_of`` [B] the palette entry of each vehicle.  local_position, global_position, lpv,
        estimate_abc, solve* and a lap-0 fleet started with ``cl_init(..., tyre_params=...)`` (``"linear"``: no tyre rows) then take
        vehicle b's track, must have batch size B, and take each track's half width and slack instead of the call's.  ``None``
        unbinds.  ``handoff`` and a race started with ``race_init(..., tyre_params=...)`` on three engines with equal bindings take
        it too.  The other ``cl_init`` / ``race_init`` starts and the cascade refuse a bound engine."""
        if maps is None:
            self._chk(self._lib.lpvmpc_set_tracks(self._h, 0, None, None, None, None, 0, None))
            return
        from .track import pack_tracks
        rows, tab, hw, sl, of = pack_tracks(maps, track_of)
        self._chk(self._lib.lpvmpc_set_tracks(self._h, rows.shape[0], ptr(rows), ptr(tab), ptr(hw), ptr(sl), of.shape[0], ptr(of)))

    def tracks_read(self):
        """The bound tracks as they were set (lpvmpc_tracks_read): dict(tables = list of T PointAndTangent arrays [rows, 6],
        half_width [T], slack [T], track_of [B]), or None while nothing is bound."""
        T, B = C.c_int32(0), C.c_int32(0)
        self._chk(self._lib.lpvmpc_tracks_read(self._h, C.byref(T), C.byref(B), None, None, None, None, None))
        if T.value == 0:
            return None
        rows, of = np.empty(T.value, np.int32), np.empty(B.value, np.int32)
        tab, hw, sl = np.empty((T.value, _ffi.MAX_TRACK_ROWS, 6)), np.empty(T.value), np.empty(T.value)
        self._chk(self._lib.lpvmpc_tracks_read(self._h, C.byref(T), C.byref(B), ptr(rows), ptr(tab), ptr(hw), ptr(sl), ptr(of)))
        return dict(tables=[tab[t, :rows[t]].copy() for t in range(T.value)], half_width=hw, slack=sl, track_of=of)

    def set_tunings(self, rows):
        """Bind per-instance tuning rows [B, 64] (tuning.py: Q, R, dR, L_cf and the limits) to this engine (lpvmpc_set_tunings): every
        call that solves -- solve, solve_AB, solve_batch_masked, solve_dev, and a fleet, cascade or race started afterwards -- then
        builds instance b's QP with row b instead of the engine's own tuning and must have batch size B.  ``None`` unbinds.  Refused
        while the engine runs a fleet, cascade or race."""
        if rows is None:
            self._chk(self._lib.lpvmpc_set_tunings(self._h, 0, None))
            return
        a = np.asarray(rows)
        if a.ndim != 2 or a.shape[0] < 1:
            raise ValueError("tunings has shape %s, expected (B, %d) with B >= 1" % (a.shape, _ffi.TUNING_WORDS))
        from .tuning import check_tuning_rows
        a = check_tuning_rows(a, a.shape[0], self.kind)
        self._chk(self._lib.lpvmpc_set_tunings(self._h, a.shape[0], ptr(a)))

    def tunings_read(self):
        """The bound tuning rows [B, 64] as they were set (lpvmpc_tunings_read), or None while nothing is bound."""
        B = C.c_int32(0)
        self._chk(self._lib.lpvmpc_tunings_read(self._h, C.byref(B), None))
        if B.value == 0:
            return None
        out = np.empty((B.value, _ffi.TUNING_WORDS))
        self._chk(self._lib.lpvmpc_tunings_read(self._h, C.byref(B), ptr(out)))
        return out

    def cl_init(self, plant0, half_width, slack, q9_swap=True, n_sub=7, dt_sim=0.005, mu_sim=0.05, actuator=None, delay_a=None,
                delay_df=None, plant_params=None, tyre_params=None):
        """Start a lap-0 fleet.  ``actuator`` (an ``actuator.actuator_config`` result, even an all-off one) selects
        lpvmpc_cl_init_actuated: the actuator in the plant, controllers of any steering delay, per-vehicle delays delay_a /
        delay_df [B] in steps (None: the config's).  Without it the call is lpvmpc_cl_init.  ``plant_params`` [B, 7] (or
        "nominal": the nominal rows) selects lpvmpc_cl_init_vehicles: each vehicle's plant steps with its own row (lf, lr, m, Iz,
        Cf, Cr, mu; mu_sim is then ignored), the actuator all off unless ``actuator`` is given.  ``tyre_params`` [B, 4] = (kind, B,
        C, c_f) per vehicle, or "pacejka", selects lpvmpc_cl_init_tyres: the same fleet (plant_params None: nominal rows) whose kind
        1 vehicles step with Simulator.pacejka on both axles.  With an estimator attached, a per-vehicle estimator bound to the
        engine (``set_observer_vehicles``) runs in the fleets started with ``plant_params`` / ``tyre_params``; the other starts
        refuse it."""
        p0 = f64(plant0).reshape(-1, 8)
        if plant_params is not None or tyre_params is not None:
            B = p0.shape[0]
            rows = None if plant_params is None or _is_nominal(plant_params) else _plant_rows(plant_params, B)
            la, ld = _delay_array(delay_a, B, "delay_a"), _delay_array(delay_df, B, "delay_df")
            if actuator is None and (la is not None or ld is not None):
                raise ValueError("per-vehicle delays need an actuator config")
            if tyre_params is not None:
                tyres = _tyre_rows(tyre_params, B)
                self._chk(self._lib.lpvmpc_cl_init_tyres(self._h, B, ptr(p0), float(half_width), float(slack), 1 if q9_swap else 0,
                                                         int(n_sub), float(dt_sim), float(mu_sim),
                                                         None if actuator is None else C.byref(_actuator_cfg(actuator)),
                                                         ptr(la), ptr(ld), ptr(rows), ptr(tyres)))
                self._cl_B = B
                return
            self._cl_B = B
            self._chk(self._lib.lpvmpc_cl_init_vehicles(self._h, B, ptr(p0), float(half_width), float(slack), 1 if q9_swap else 0,
                                                        int(n_sub), float(dt_sim), float(mu_sim),
                                                        None if actuator is None else C.byref(_actuator_cfg(actuator)),
                                                        ptr(la), ptr(ld), ptr(rows)))
            return
        self._cl_B = p0.shape[0]
        if actuator is None:
            if delay_a is not None or delay_df is not None:
                raise ValueError("per-vehicle delays need an actuator config")
            self._chk(self._lib.lpvmpc_cl_init(self._h, self._cl_B, ptr(p0), float(half_width), float(slack), 1 if q9_swap else 0,
                                               int(n_sub), float(dt_sim), float(mu_sim)))
        else:
            la, ld = _delay_array(delay_a, self._cl_B, "delay_a"), _delay_array(delay_df, self._cl_B, "delay_df")
            self._chk(self._lib.lpvmpc_cl_init_actuated(self._h, self._cl_B, ptr(p0), float(half_width), float(slack), 1 if q9_swap else 0,
                                                        int(n_sub), float(dt_sim), float(mu_sim), C.byref(_actuator_cfg(actuator)),
                                                        ptr(la), ptr(ld)))

    def actuator_read(self):
        """Of a fleet / race started with ``actuator``: act_state [B, ACT_WORDS] and the controllers' u_old histories [B, 2 + d] =
        [OldSteering[0], OldAccelera[0], OldSteering[1..d]] ("path"; a race also "tt").  A lap-0 fleet's history is what its next
        solve reads, a race's what its last solve read (include/lpvmpc.h)."""
        race = getattr(self, "_race", None) is not None
        B = self._race[0] if race else self._cl_B
        d = int(self.cfg.steering_delay)
        o = dict(act_state=np.empty((B, _ffi.ACT_WORDS)), path=np.empty((B, 2 + d)))
        if race:
            o["tt"] = np.empty((B, 2 + d))
        self._chk(self._lib.lpvmpc_actuator_read(self._h, ptr(o["act_state"]), ptr(o["path"]), ptr(o.get("tt"))))
        return o

    def cl_tick(self, n_ticks=1):
        self._chk(self._lib.lpvmpc_cl_tick(self._h, int(n_ticks)))

    def cl_read(self):
        B = self._cl_B
        o = dict(plant=np.empty((B, 8)), local=np.empty((B, 6)), cmd=np.empty((B, 2)), iters=np.empty(B, np.int32),
                 status=np.empty(B, np.int32))
        self._chk(self._lib.lpvmpc_cl_read(self._h, ptr(o["plant"]), ptr(o["local"]), ptr(o["cmd"]), ptr(o["iters"]), ptr(o["status"])))
        return o

    # -- gain-scheduled LPV estimator (lpvmpc_observer_*) ------------------------------------------------------
    def observer_setup(self, cfg=None, **kw):
        """Attach the estimator to this CONTROLLER engine's next cl_init or cascade_init (``cfg``: an ``observer.observer_config`` result or an
        ``_ffi.ObserverConfig``; keyword arguments build one with ``observer.observer_config``).  ``observer_setup(None)``
        removes it: the next fleet runs on ground truth again."""
        if cfg is None and kw:
            from .observer import observer_config
            cfg = observer_config(**kw)
        self._chk(self._lib.lpvmpc_observer_setup(self._h, None if cfg is None else C.byref(cfg)))

    def observer_read(self):
        """The fleet's (or cascade's, or race's) estimate [B,6] = [vx vy psiDot x y yaw] and latest measurement [B,5] =
        [vx psiDot x y yaw]."""
        if getattr(self, "_race", None) is not None:
            B = self._race[0]
        elif getattr(self, "_cas", None) is not None:
            B = self._cas[0]
        else:
            B = getattr(self, "_cl_B", 0)
        est, meas = np.empty((B, 6)), np.empty((B, 5))
        self._chk(self._lib.lpvmpc_observer_read(self._h, ptr(est), ptr(meas)))
        return est, meas

    def observer_step(self, cfg, est, y, u, k, want_aux=False):
        """One GS_LPV_Est step per instance: est [B,6], y [B,5], u [B,2] = (servo, motor), k [B] (t = k / loop_rate).
        Returns the new estimate, and with ``want_aux`` also (L_gain [B,6,5], A_obs [B,6,6], B_obs [B,6,2])."""
        e = f64(est).reshape(-1, 6).copy()
        B = e.shape[0]
        y = f64(y, (B, 5), "y"); u = f64(u, (B, 2), "u")
        k = np.ascontiguousarray(np.broadcast_to(np.asarray(k, np.int32), (B,)))
        aux = np.empty((B, _ffi.OBSERVER_AUX)) if want_aux else None
        self._chk(self._lib.lpvmpc_observer_step_batch(self._h, B, C.byref(cfg), ptr(e), ptr(y), ptr(u), ptr(k), ptr(aux)))
        if not want_aux:
            return e
        return e, (aux[:, :30].reshape(B, 6, 5), aux[:, 30:66].reshape(B, 6, 6), aux[:, 66:].reshape(B, 6, 2))

    def observer_design(self, rows, lim_ls, lim_hs, Qo=None, Ro=None, want_iters=False, out=None):
        """Vertex gains of the estimator designed on the device for each vehicle's model row: rows [B,7] = (lf, lr, m, Iz, Cf, Cr,
        mu), the two SchedVars_Limits tables [6,2]; Qo [6,6] and Ro [5,5] default to ``observer.observer_vertex_gains``' weights.
        Returns (L_ls [B,6,5,16], L_hs [B,6,5,16]) and with ``want_iters`` the Newton iterations [B,2,16] as well (-1 with NaN gains:
        not converged).  ``out``: a pair of arrays to fill instead of new ones."""
        rows = f64(rows).reshape(-1, _ffi.PLANT_WORDS)
        B = rows.shape[0]
        d = observer_design_config(lim_ls, lim_hs, Qo, Ro)
        L_ls, L_hs = out if out is not None else (np.empty((B, 6, 5, 16)), np.empty((B, 6, 5, 16)))
        iters = np.empty((B, 2, 16), np.int32) if want_iters else None
        self._chk(self._lib.lpvmpc_observer_design_batch(self._h, B, ptr(rows), C.byref(d), ptr(L_ls), ptr(L_hs), ptr(iters)))
        return (L_ls, L_hs, iters) if want_iters else (L_ls, L_hs)

    def set_observer_vehicles(self, rows, L_ls=None, L_hs=None, design=None):
        """Bind a per-vehicle estimator to this CONTROLLER engine (for a race: the path engine): model rows [B,7] and either the gain
        tables ``L_ls``, ``L_hs`` [B,6,5,16] or ``design`` -- an ``observer_design_config`` result or a dict of its arguments
        (lim_ls, lim_hs, Qo, Ro) -- for tables designed on the device straight into the binding.  The estimator of a fleet or race
        started with per-vehicle rows (``cl_init(plant_params=...)``, ``race_init(plant_params=...)``) then runs each vehicle's
        observer step on its own row and tables.  ``set_observer_vehicles(None)`` unbinds."""
        if rows is None:
            self._chk(self._lib.lpvmpc_set_observer_vehicles(self._h, 0, None, None, None, None))
            return
        rows = f64(rows).reshape(-1, _ffi.PLANT_WORDS)
        B = rows.shape[0]
        if isinstance(design, dict):
            design = observer_design_config(**design)
        L_ls = None if L_ls is None else f64(L_ls, (B, 6, 5, 16), "L_ls")
        L_hs = None if L_hs is None else f64(L_hs, (B, 6, 5, 16), "L_hs")
        self._chk(self._lib.lpvmpc_set_observer_vehicles(self._h, B, ptr(rows), ptr(L_ls), ptr(L_hs),
                                                         None if design is None else C.byref(design)))

    def observer_vehicles_read(self):
        """The bound per-vehicle estimator as (rows [B,7], L_ls [B,6,5,16], L_hs [B,6,5,16]), or None when nothing is bound."""
        n = C.c_int32(0)
        self._chk(self._lib.lpvmpc_observer_vehicles_read(self._h, C.byref(n), None, None, None))
        if n.value == 0:
            return None
        rows, L_ls, L_hs = np.empty((n.value, _ffi.PLANT_WORDS)), np.empty((n.value, 6, 5, 16)), np.empty((n.value, 6, 5, 16))
        self._chk(self._lib.lpvmpc_observer_vehicles_read(self._h, C.byref(n), ptr(rows), ptr(L_ls), ptr(L_hs)))
        return rows, L_ls, L_hs

    def observer_step_vehicles(self, cfg, est, y, u, k, rows, L_ls, L_hs, want_aux=False):
        """``observer_step`` with a model row [B,7] and gain tables [B,6,5,16] per instance (cfg's own tables are ignored)."""
        e = f64(est).reshape(-1, 6).copy()
        B = e.shape[0]
        y = f64(y, (B, 5), "y"); u = f64(u, (B, 2), "u")
        k = np.ascontiguousarray(np.broadcast_to(np.asarray(k, np.int32), (B,)))
        rows = f64(rows, (B, _ffi.PLANT_WORDS), "rows"); L_ls = f64(L_ls, (B, 6, 5, 16), "L_ls"); L_hs = f64(L_hs, (B, 6, 5, 16), "L_hs")
        aux = np.empty((B, _ffi.OBSERVER_AUX)) if want_aux else None
        self._chk(self._lib.lpvmpc_observer_step_vehicles_batch(self._h, B, C.byref(cfg), ptr(e), ptr(y), ptr(u), ptr(k), ptr(aux),
                                                                ptr(rows), ptr(L_ls), ptr(L_hs)))
        if not want_aux:
            return e
        return e, (aux[:, :30].reshape(B, 6, 5), aux[:, 30:66].reshape(B, 6, 6), aux[:, 66:].reshape(B, 6, 2))

    # -- planner -> controller hand-off ------------------------------------------------
    def handoff_setup(self, cfg=None):
        """Build the resampling / filtering operators for this PLANNER handle; returns M (samples per My_Planning array)."""
        cfg = cfg if cfg is not None else _ffi.default_handoff_config()
        M = self._lib.lpvmpc_handoff_setup(self._h, C.byref(cfg))
        self._chk(min(M, 0))
        self._ho_M = M
        return M

    def handoff(self, xPred, SS, pose, want_sig=False):
        """PMAIN:201-224,257-308 for a batch.  Returns dict(SS, pose, refs[, sig]); SS / pose are the carried state."""
        N = self.N
        x = f64(xPred).reshape(-1, N + 1, 5)
        B = x.shape[0]
        SS = f64(SS, (B, N + 1), "SS").copy(); pose = f64(pose, (B, 3), "pose").copy()
        refs = np.empty((B, 5, self._ho_M)); sig = np.empty((B, 5, N)) if want_sig else None
        self._chk(self._lib.lpvmpc_handoff_batch(self._h, B, ptr(x), ptr(SS), ptr(pose), ptr(sig), ptr(refs)))
        out = dict(SS=SS, pose=pose, refs=refs)
        if want_sig:
            out["sig"] = sig
        return out

    # -- planner + controller + plant cascade (configs[4]) ------------------------------------------------
    def cl_release(self):
        """End the closed-loop fleet / cascade of this engine: batch calls are accepted again (they are refused while a fleet
        runs, because the fleet's state lives in the engine's workspace)."""
        self._chk(self._lib.lpvmpc_cl_release(self._h))
        self._cas = None
        self._cas_planner = None
        self._race = None
        self._rec = None

    def cascade_init(self, planner, plant0, cmd0, uPred0, lap0=1, half_width=0.3, slack=0.15, plan_max_ey=0.2, q9_swap=True,
                     n_sub=(7, 7, 6), dt_sim=0.005, mu_sim=0.05):
        p0 = f64(plant0).reshape(-1, 8)
        B = p0.shape[0]
        c0 = f64(cmd0, (B, 2), "cmd0"); u0 = f64(uPred0, (B, self.N, 2), "uPred0")
        ns = np.ascontiguousarray(n_sub, np.int32)
        if ns.shape != (3,):
            raise ValueError("n_sub must have 3 entries")
        self._chk(self._lib.lpvmpc_cascade_init(self._h, planner._h, B, ptr(p0), ptr(c0), ptr(u0), int(lap0), float(half_width),
                                                float(slack), float(plan_max_ey), 1 if q9_swap else 0, ptr(ns), float(dt_sim), float(mu_sim)))
        self._cas = (B, planner.N, planner._ho_M)
        self._cas_planner = planner                      # keep the planner handle alive as long as the cascade

    def cascade_tick(self, n_ticks=1):
        self._chk(self._lib.lpvmpc_cascade_tick(self._h, int(n_ticks)))

    def cascade_read(self, full=True):
        if self._cas is None:
            raise LpvMpcError(_ffi.E_ARG, "cascade_read: call cascade_init first")
        B, Np, M = self._cas
        o = dict(plant=np.empty((B, 8)), local=np.empty((B, 6)), cmd=np.empty((B, 2)), iters=np.empty(B, np.int32),
                 status=np.empty(B, np.int32), lap=np.empty(B, np.int32), lap_tick=np.empty(B, np.int32),
                 plan_iters=np.empty(B, np.int32), plan_status=np.empty(B, np.int32), ticks=np.empty(2, np.int32))
        if full:
            o.update(refs=np.empty((B, 5, M)), plan_xPred=np.empty((B, Np + 1, 5)))
        self._chk(self._lib.lpvmpc_cascade_read(self._h, ptr(o["plant"]), ptr(o["local"]), ptr(o["cmd"]), ptr(o["iters"]), ptr(o["status"]),
                                                ptr(o["lap"]), ptr(o["lap_tick"]), ptr(o.get("refs")), ptr(o.get("plan_xPred")),
                                                ptr(o["plan_iters"]), ptr(o["plan_status"]), ptr(o["ticks"])))
        return o

    def cascade_alive_ticks(self):
        """Controller ticks each vehicle of the cascade has entered with a finite plant state ([B] int32)."""
        if self._cas is None:
            raise LpvMpcError(_ffi.E_ARG, "cascade_alive_ticks: call cascade_init first")
        out = np.empty(self._cas[0], np.int32)
        self._chk(self._lib.lpvmpc_cascade_alive_ticks(self._h, ptr(out)))
        return out

    # -- race engine: lap 0, per-vehicle lap events, racing (lpvmpc_race_*) ------------------------------------
    def race_init(self, tt, planner, plant0, half_track0=None, estimator=None, actuator=None, delay_a=None, delay_df=None, plant_params=None,
                  tyre_params=None, **cfg):
        """Start a race owned by this PATH controller engine, with ``tt`` (racing tuning) and ``planner`` (handoff_setup done).
        plant0 [B,8]; half_track0 [B] (HalfTrack at the start, default 0); ``cfg``: fields of ``lpvmpc_race_config`` (laps,
        n_sub_lap0, n_sub, q9_swap, half_width, slack, plan_max_ey, dt_sim, mu_sim).  ``estimator``: an
        ``observer.observer_config`` result or an ``_ffi.ObserverConfig`` runs the race with the state estimator and the
        simulated sensors in the loop (lpvmpc_race_init_observed; ``observer_read`` then returns its state); None runs it on
        ground truth.  ``actuator`` (an ``actuator.actuator_config`` result, even an all-off one) selects lpvmpc_race_init_actuated:
        the actuator in the plant, path / tt of the same steering delay, per-vehicle delays delay_a / delay_df [B] in steps.
        ``plant_params`` [B, 7] (or "nominal") selects lpvmpc_race_init_vehicles: each vehicle's plant steps with its own row (lf,
        lr, m, Iz, Cf, Cr, mu; cfg mu_sim is then ignored), with or without ``estimator`` / ``actuator``.  ``tyre_params`` [B, 4] =
        (kind, B, C, c_f) per vehicle, or "pacejka", selects lpvmpc_race_init_tyres: the same race (plant_params None: nominal rows)
        whose kind 1 vehicles step with Simulator.pacejka on both axles.  With ``estimator``, a per-vehicle estimator bound to this
        (path) engine (``set_observer_vehicles``) runs in the races started with ``plant_params`` / ``tyre_params``; the other
        starts refuse it."""
        p0 = f64(plant0).reshape(-1, 8)
        B = p0.shape[0]
        c = _ffi.default_race_config()
        for k, v in cfg.items():
            if k == "n_sub":
                v = list(v)
                if len(v) != 3:
                    raise ValueError("n_sub must have 3 entries")
                for i in range(3):
                    c.n_sub[i] = int(v[i])
            elif k in ("laps", "n_sub_lap0", "q9_swap"):
                setattr(c, k, int(v))
            elif k in ("half_width", "slack", "plan_max_ey", "dt_sim", "mu_sim"):
                setattr(c, k, float(v))
            else:
                raise TypeError("unknown race option %r" % k)
        ht = None if half_track0 is None else np.ascontiguousarray(np.broadcast_to(np.asarray(half_track0), (B,)), np.int32)
        if estimator is not None and not isinstance(estimator, _ffi.ObserverConfig):
            raise TypeError("estimator must be an observer.observer_config(...) result or an _ffi.ObserverConfig")
        if plant_params is not None or tyre_params is not None:
            rows = None if plant_params is None or _is_nominal(plant_params) else _plant_rows(plant_params, B)
            la, ld = _delay_array(delay_a, B, "delay_a"), _delay_array(delay_df, B, "delay_df")
            if actuator is None and (la is not None or ld is not None):
                raise ValueError("per-vehicle delays need an actuator config")
            args = (self._h, tt._h, planner._h, B, ptr(p0), ptr(ht), C.byref(c), None if estimator is None else C.byref(estimator),
                    None if actuator is None else C.byref(_actuator_cfg(actuator)), ptr(la), ptr(ld), ptr(rows))
            if tyre_params is not None:
                self._chk(self._lib.lpvmpc_race_init_tyres(*(args + (ptr(_tyre_rows(tyre_params, B)),))))
            else:
                self._chk(self._lib.lpvmpc_race_init_vehicles(*args))
        elif actuator is not None:
            la, ld = _delay_array(delay_a, B, "delay_a"), _delay_array(delay_df, B, "delay_df")
            self._chk(self._lib.lpvmpc_race_init_actuated(self._h, tt._h, planner._h, B, ptr(p0), ptr(ht), C.byref(c),
                                                          None if estimator is None else C.byref(estimator), C.byref(_actuator_cfg(actuator)),
                                                          ptr(la), ptr(ld)))
        elif delay_a is not None or delay_df is not None:
            raise ValueError("per-vehicle delays need an actuator config")
        elif estimator is None:
            self._chk(self._lib.lpvmpc_race_init(self._h, tt._h, planner._h, B, ptr(p0), ptr(ht), C.byref(c)))
        else:
            if not isinstance(estimator, _ffi.ObserverConfig):
                raise TypeError("estimator must be an observer.observer_config(...) result or an _ffi.ObserverConfig")
            self._chk(self._lib.lpvmpc_race_init_observed(self._h, tt._h, planner._h, B, ptr(p0), ptr(ht), C.byref(c), C.byref(estimator)))
        self._race = (B, int(c.laps), tt, planner)           # (keeps the two other engines alive as long as the race)
        self._rec = None

    def race_tick(self, n_ticks=1):
        self._chk(self._lib.lpvmpc_race_tick(self._h, int(n_ticks)))

    def _race_B(self, who):
        if self._race is None:
            raise LpvMpcError(_ffi.E_ARG, "%s: call race_init first" % who)
        return self._race[0]

    def race_read(self):
        """Synchronise and return the fleet: plant, local, cmd, phase (0 lap 0, 1 racing, 2 finished, 3 lost), lap, iters / status
        (the vehicle's controller solve of the last tick; iters 0 when it did not solve), plan_iters / plan_status, ticks."""
        B = self._race_B("race_read")
        o = dict(plant=np.empty((B, 8)), local=np.empty((B, 6)), cmd=np.empty((B, 2)), phase=np.empty(B, np.int32),
                 lap=np.empty(B, np.int32), iters=np.empty(B, np.int32), status=np.empty(B, np.int32),
                 plan_iters=np.empty(B, np.int32), plan_status=np.empty(B, np.int32))
        t = np.zeros(1, np.int32)
        self._chk(self._lib.lpvmpc_race_read(self._h, ptr(o["plant"]), ptr(o["local"]), ptr(o["cmd"]), ptr(o["phase"]), ptr(o["lap"]),
                                             ptr(o["iters"]), ptr(o["status"]), ptr(o["plan_iters"]), ptr(o["plan_status"]), ptr(t)))
        o["ticks"] = int(t[0])
        return o

    def race_laps(self):
        """lap_step [B, laps+2] (plant step at which each lap started, -1 not yet) and alive_ticks [B]."""
        B = self._race_B("race_laps")
        ls = np.empty((B, self._race[1] + 2), np.int32); al = np.empty(B, np.int32)
        self._chk(self._lib.lpvmpc_race_laps(self._h, ptr(ls), ptr(al)))
        return ls, al

    def race_predictions(self):
        """(path uPred, tt uPred), each [B, N, 2]: the u_prev of the two controllers' next roll-out."""
        B = self._race_B("race_predictions")
        pu = np.empty((B, self.N, 2)); tu = np.empty((B, self.N, 2))
        self._chk(self._lib.lpvmpc_race_predictions(self._h, ptr(pu), ptr(tu)))
        return pu, tu

    def race_record(self, capacity, stride=1):
        """Record the race from the next tick on (lpvmpc_race_record): a ring of the last ``capacity`` records, one every
        ``stride`` ticks, and the per-lap statistics of every tick.  Restarting resets both; ``capacity`` 0 stops recording."""
        self._race_B("race_record")
        cfg = _ffi.RaceRecordConfig(int(capacity), int(stride))
        try:
            self._chk(self._lib.lpvmpc_race_record(self._h, C.byref(cfg)))
        except LpvMpcError as e:
            if e.code != _ffi.E_ARG:                 # (a refused argument leaves the recorder as it was; a failed allocation stops it)
                self._rec = None
            raise
        self._rec = (int(capacity), int(stride)) if capacity else None

    def race_record_read(self, last=None):
        """The last ``last`` (default: all kept) records, oldest first: a dict of [n, B] arrays named as _ffi.REC_F64_NAMES /
        REC_I32_NAMES, the same channels grouped (plant [n,B,8], local [n,B,6], cmd [n,B,2], ref [n,B,4], track [n,B,3],
        est [n,B,6]), tick [n] and total (records written since recording started)."""
        B = self._race_B("race_record_read")
        if last is not None and int(last) < 0:               # the library's refusal
            self._chk(self._lib.lpvmpc_race_record_read(self._h, int(last), None, None, None, None))
        rec = getattr(self, "_rec", None)
        cap = rec[0] if rec else 0
        n = cap if last is None else min(int(last), cap)
        f = np.empty((n, _ffi.REC_F64, B)); i = np.empty((n, _ffi.REC_I32, B), np.int32); tick = np.empty(n, np.int32)
        total = np.zeros(1, np.int32)
        self._chk(self._lib.lpvmpc_race_record_read(self._h, n, ptr(total), ptr(tick), ptr(f), ptr(i)))
        m = min(n, int(total[0]))                        # records copied (n <= capacity)
        f, i, tick = f[:m], i[:m], tick[:m]
        out = {k: f[:, c] for c, k in enumerate(_ffi.REC_F64_NAMES)}
        out.update({k: i[:, c] for c, k in enumerate(_ffi.REC_I32_NAMES)})
        for k, c, w in (("plant", _ffi.REC_PLANT, 8), ("local", _ffi.REC_LOCAL, 6), ("cmd", _ffi.REC_CMD, 2), ("ref", _ffi.REC_REF, 4),
                        ("track", _ffi.REC_TRACK, 3), ("est", _ffi.REC_EST, 6)):
            out[k] = np.ascontiguousarray(f[:, c:c + w].transpose(0, 2, 1))
        out["tick"] = tick
        out["total"] = int(total[0])
        return out

    def race_lap_stats(self):
        """Per-lap statistics of the recorded ticks: a dict of [B, laps+1] arrays named as _ffi.LAPSTAT_F64_NAMES /
        LAPSTAT_I32_NAMES, the raw planes f64 [B, laps+1, 6] / i32 [B, laps+1, 9], and end_tick [B]."""
        B = self._race_B("race_lap_stats")
        L1 = self._race[1] + 1
        f = np.empty((B, L1, _ffi.LAPSTAT_F64)); i = np.empty((B, L1, _ffi.LAPSTAT_I32), np.int32); e = np.empty(B, np.int32)
        self._chk(self._lib.lpvmpc_race_lap_stats(self._h, ptr(f), ptr(i), ptr(e)))
        return _ffi.lap_stats_dict(f, i, e)

    # -- race snapshot, restore and clone (lpvmpc_race_snapshot / _restore / _clone; snapshot.py) -----------------
    def race_snapshot(self, raw=False):
        """Synchronise and return the race's whole per-vehicle state and tick counter as a ``snapshot.RaceSnapshot`` (``raw``: the
        blob's bytes).  It carries state only: bindings (plant, tyre, model, tuning, track, gain and disturbance rows) are the
        caller's business.  Changes nothing; allowed while recording."""
        from .snapshot import RaceSnapshot
        self._race_B("race_snapshot")
        n = C.c_int64(0)
        self._chk(self._lib.lpvmpc_race_snapshot_size(self._h, C.byref(n)))
        buf = np.empty(n.value, np.uint8)
        self._chk(self._lib.lpvmpc_race_snapshot(self._h, ptr(buf), n.value))
        blob = buf.tobytes()
        return blob if raw else RaceSnapshot.from_bytes(blob)

    def race_restore(self, snap):
        """Put a snapshot (a ``RaceSnapshot`` or a blob's bytes) back into this race: the one it came from, or a freshly initialised
        one of the same shape and features with the same bindings.  Refused (LpvMpcError, the race untouched) where header or
        directory differ from the live race's, and while a recorder is attached."""
        self._race_B("race_restore")
        blob = snap.to_bytes() if hasattr(snap, "to_bytes") else bytes(snap)
        buf = np.frombuffer(blob, np.uint8)
        self._chk(self._lib.lpvmpc_race_restore(self._h, ptr(buf), len(blob)))

    def race_clone(self, src):
        """Vehicle b takes the whole state of vehicle src[b] and keeps its own bindings (src [B]; duplicates, swaps and cycles read
        the state before the call).  Returns the number of vehicles moved.  Refused, with nothing changed: an index outside [0, B),
        a source on another track of a track-bound race, a recorder attached."""
        B = self._race_B("race_clone")
        s = np.ascontiguousarray(np.asarray(src).reshape(-1), np.int32)
        if s.shape[0] != B:
            raise ValueError("race_clone: src must have one entry per vehicle (%d), got %d" % (B, s.shape[0]))
        moved = _ffi._i(0)
        self._chk(self._lib.lpvmpc_race_clone(self._h, ptr(s), C.byref(moved)))
        return int(moved.value)

    # -- heats: standings, gaps, passes and contacts (lpvmpc_race_heats / _standings, lpvmpc_heat_step_batch; heats.py) ----
    def race_heats(self, heat, turns0=None, half_length=0.4, half_width=0.2):
        """Attach heats from the next tick on (lpvmpc_race_heats): ``heat`` [B], the heat of each vehicle (-1: none; at most 256
        members each; with tracks bound, one track per heat), ``turns0`` [B] the starting turn count (default 0; -1 for a car gridded
        behind the line), ``half_length`` / ``half_width`` the half extents of a car's footprint.  Re-attaching resets the standings;
        ``heat=None`` detaches.  Heats only observe: no output of the race changes."""
        B = self._race_B("race_heats")
        if heat is None:
            self._chk(self._lib.lpvmpc_race_heats(self._h, None, None, None))
            return
        cfg, h, _ = _heats_args(heat, B, None, half_length, half_width)
        t0 = None if turns0 is None else np.ascontiguousarray(np.asarray(turns0).reshape(-1), np.int32)
        if t0 is not None and t0.shape[0] != B:
            raise ValueError("race_heats: turns0 must have one entry per vehicle (%d), got %d" % (B, t0.shape[0]))
        self._chk(self._lib.lpvmpc_race_heats(self._h, C.byref(cfg), ptr(h), ptr(t0)))

    def race_standings(self):
        """Synchronise and return the standings (lpvmpc_race_standings): a dict of [B] arrays named as _ffi.HEAT_F64_NAMES /
        HEAT_I32_NAMES (progress, gap_ahead, gap_leader, clearance, min_clearance; position, ahead, nearest, contact, contact_ticks,
        first_contact_tick, passes, passed, turns, class), the planes f64 [5, B] / i32 [10, B], and line_tick / line_pos
        [B, laps + 2].  A vehicle in no heat reads position -1 and NaN gaps."""
        from . import heats as H
        B = self._race_B("race_standings")
        K = self._race[1] + 2
        lt = np.empty((B, K), np.int32); lp = np.empty((B, K), np.int32)
        f, i = _read_planes(self, self._lib.lpvmpc_race_standings, B, _ffi.HEAT_F64, _ffi.HEAT_I32, lt, lp)
        return H.standings_dict(f, i, lt, lp)

    def heat_step(self, heat, L, pose, s, inside, phase, t, carry=None, n_heats=None, half_length=0.4, half_width=0.2):
        """One tick of the heats' device function on the caller's data (lpvmpc_heat_step_batch): ``heat`` [B] (-1: none), ``L`` [B]
        (or one value) each vehicle's track length, ``pose`` [B, 3] = x y yaw, ``s`` / ``inside`` [B] the track frame, ``phase`` [B],
        ``t`` the tick number.  ``carry``: the state returned by the previous call (None: ``heats.new_carry(B)``, just attached).
        Returns (standings, carry): the dict of ``race_standings`` (with the carry's line tables, if it has any) and the new carry.
        The batch form keeps no line tables on the device: the kernel carries the count of lines crossed, and the tables of a carry made
        with ``heats.new_carry(..., lines=K)`` are filled HERE, on the host, from that count and this tick's position -- a convenience
        that mirrors what the race's kernel writes on the device (``race_standings``), not a read-back of it."""
        from . import heats as H
        pose = f64(pose)
        if pose.ndim != 2 or pose.shape[1] != 3:
            raise ValueError("heat_step: pose must be [B, 3], got %s" % (pose.shape,))
        B = pose.shape[0]
        cfg, h, n = _heats_args(heat, B, n_heats, half_length, half_width)
        Lb = f64(np.broadcast_to(np.asarray(L, float), (B,)), (B,), "L")
        s = f64(s, (B,), "s")
        ins = np.ascontiguousarray(np.asarray(inside).reshape(-1), np.int32)
        ph = np.ascontiguousarray(np.asarray(phase).reshape(-1), np.int32)
        if ins.shape[0] != B or ph.shape[0] != B:
            raise ValueError("heat_step: inside and phase must have one entry per vehicle (%d)" % B)
        c = H.new_carry(B) if carry is None else carry
        cf, ci = _carry_in("heat_step", c, _ffi.HEAT_CARRY_F64, _ffi.HEAT_CARRY_I32, B)
        f = np.empty((_ffi.HEAT_F64, B)); i = np.empty((_ffi.HEAT_I32, B), np.int32)
        was = ci[_ffi.HEAT_CARRY_I32_NAMES.index("crossings")].copy() * (ci[0] & 1)
        self._chk(self._lib.lpvmpc_heat_step_batch(self._h, B, n, ptr(h), ptr(Lb), C.byref(cfg), int(t), ptr(pose), ptr(s), ptr(ins), ptr(ph),
                                                   ptr(cf), ptr(ci), ptr(f), ptr(i)))
        out = dict(f64=cf, i32=ci)
        lt = lp = None
        if "line_tick" in c:                                   # the line tables, filled as the race's kernel fills them on the device
            lt, lp = c["line_tick"].copy(), c["line_pos"].copy()
            if not (c["i32"][0] & 1).any():
                lt[h >= 0] = -1; lp[h >= 0] = -1
            now = ci[_ffi.HEAT_CARRY_I32_NAMES.index("crossings")]
            for b in np.nonzero((h >= 0) & (now > was) & (was < lt.shape[1]))[0]:
                lt[b, was[b]] = int(t); lp[b, was[b]] = i[_ffi.HEAT_I32_NAMES.index("position"), b]
            out.update(line_tick=lt, line_pos=lp)
        return H.standings_dict(f, i, lt, lp), out

    # -- interactions: slipstream and contact response within a heat (lpvmpc_race_interactions / _read, lpvmpc_interaction_step_batch;
    # interactions.py) --------------------------------------------------------------------------------------------------------
    def race_interactions(self, cfg=None, detach=False):
        """Attach the interactions from the next tick on (lpvmpc_race_interactions): ``cfg`` an ``interactions.interaction_config(...)``
        result, a dict of its words, or None for the defaults.  Needs heats attached (``race_heats``) and a race started with
        ``plant_params`` / ``tyre_params``.  Attaching again replaces the binding; ``detach=True`` detaches and puts the base mu words
        back into the live plant table.  ``race_heats`` detaches the interactions, whether it re-attaches or detaches the heats."""
        from . import interactions as I
        self._race_B("race_interactions")
        _race_attach(self, self._lib.lpvmpc_race_interactions, None if detach else I.as_config(cfg))

    def race_interactions_read(self):
        """Synchronise and return the interactions' outputs (lpvmpc_race_interactions_read): a dict of [B] arrays named as
        _ffi.INTER_F64_NAMES / INTER_I32_NAMES (shelter, mu, impulse, impulse_total; leader, hit, hit_ticks, first_hit_tick,
        draft_ticks) and the planes f64 [4, B] / i32 [5, B].  A vehicle in no heat reads NaN and leader -1."""
        from . import interactions as I
        B = self._race_B("race_interactions_read")
        return I.interactions_dict(*_read_planes(self, self._lib.lpvmpc_race_interactions_read, B, _ffi.INTER_F64, _ffi.INTER_I32))

    def interaction_step(self, heat, plant, plant_params, t, cfg=None, nstep=None, carry=None, n_heats=None, half_length=0.4, half_width=0.2):
        """One tick of the interactions' kernel on the caller's data (lpvmpc_interaction_step_batch): ``heat`` [B] (-1: none), ``plant``
        [B, 8], ``plant_params`` [B, 7] (m and mu are read), ``t`` the tick number, ``cfg`` as ``race_interactions``, ``nstep`` [B] the
        simulator steps of this tick (None: every vehicle steps; 0: frozen), ``carry`` the state returned by the previous call (None:
        ``interactions.new_carry(B)``), ``half_length`` / ``half_width`` the heats' footprint.  Returns (plant [B, 8] after the tick,
        mu_live [B], outputs dict, carry)."""
        from . import interactions as I
        plant, B, rows = _step_plant("interaction_step", plant, plant_params)
        hcfg, h, n = _heats_args(heat, B, n_heats, half_length, half_width)
        c = I.as_config(cfg)
        ns = _step_nstep("interaction_step", nstep, B)
        k = I.new_carry(B) if carry is None else carry
        cf, ci = _carry_in("interaction_step", k, _ffi.INTER_CARRY_F64, _ffi.INTER_CARRY_I32, B)
        f = np.empty((_ffi.INTER_F64, B)); i = np.empty((_ffi.INTER_I32, B), np.int32); mu = np.empty(B)
        self._chk(self._lib.lpvmpc_interaction_step_batch(self._h, B, n, ptr(h), C.byref(hcfg), C.byref(c), int(t), ptr(plant), ptr(rows), ptr(ns),
                                                          ptr(cf), ptr(ci), ptr(mu), ptr(f), ptr(i)))
        return plant, mu, I.interactions_dict(f, i), dict(f64=cf, i32=ci)

    # -- contact model: the corner form of the car-to-car contact (lpvmpc_race_contact / _read, lpvmpc_contact_step_batch; contact.py) --
    def race_contact(self, cfg=None, detach=False):
        """Attach the contact model on top of the interactions from the next tick on (lpvmpc_race_contact): ``cfg`` a
        ``contact.contact_config(...)`` result, a dict of its words, or None for the defaults.  Needs interactions attached with
        ``contact=1``.  Attaching again replaces the binding; ``detach=True`` goes back to the centres form.  ``race_interactions`` and
        ``race_heats`` detach the contact model."""
        from . import contact as K
        self._race_B("race_contact")
        _race_attach(self, self._lib.lpvmpc_race_contact, None if detach else K.as_config(cfg))

    def race_contact_read(self):
        """Synchronise and return the contact model's planes (lpvmpc_race_contact_read): a dict of [B] arrays named as
        _ffi.CONTACT_F64_NAMES / CONTACT_I32_NAMES (friction_impulse, yaw_kick, yaw_kick_total; partners, max_partners) and the planes
        f64 [3, B] / i32 [2, B].  A vehicle in no heat reads NaN and 0."""
        from . import contact as K
        B = self._race_B("race_contact_read")
        return K.contact_dict(*_read_planes(self, self._lib.lpvmpc_race_contact_read, B, _ffi.CONTACT_F64, _ffi.CONTACT_I32))

    def contact_step(self, heat, plant, plant_params, t, cfg=None, contact=None, nstep=None, carry=None, contact_carry=None, n_heats=None,
                     half_length=0.4, half_width=0.2):
        """One tick of the contact model's kernel on the caller's data (lpvmpc_contact_step_batch): the arguments of
        ``interaction_step`` (``plant_params``: m, Iz and mu are read; ``cfg`` needs contact = 1) plus ``contact`` as ``race_contact``
        and ``contact_carry`` the contact model's state returned by the previous call (None: ``contact.new_contact_carry(B)``).  Returns
        (plant [B, 8] after the tick, mu_live [B], the interactions' outputs dict, their carry, the contact model's dict, its carry)."""
        from . import contact as K, interactions as I
        plant, B, rows = _step_plant("contact_step", plant, plant_params)
        hcfg, h, n = _heats_args(heat, B, n_heats, half_length, half_width)
        c = I.as_config(cfg)
        kc = K.as_config(contact)
        ns = _step_nstep("contact_step", nstep, B)
        k = I.new_carry(B) if carry is None else carry
        cf, ci = _carry_in("contact_step", k, _ffi.INTER_CARRY_F64, _ffi.INTER_CARRY_I32, B)
        kk = K.new_contact_carry(B) if contact_carry is None else contact_carry
        kf, ki = _carry_in("contact_step", kk, _ffi.CONTACT_CARRY_F64, _ffi.CONTACT_CARRY_I32, B, "contact carry")
        f = np.empty((_ffi.INTER_F64, B)); i = np.empty((_ffi.INTER_I32, B), np.int32); mu = np.empty(B)
        qf = np.empty((_ffi.CONTACT_F64, B)); qi = np.empty((_ffi.CONTACT_I32, B), np.int32)
        self._chk(self._lib.lpvmpc_contact_step_batch(self._h, B, n, ptr(h), C.byref(hcfg), C.byref(c), C.byref(kc), int(t), ptr(plant), ptr(rows),
                                                      ptr(ns), ptr(cf), ptr(ci), ptr(kf), ptr(ki), ptr(mu), ptr(f), ptr(i), ptr(qf), ptr(qi)))
        return plant, mu, I.interactions_dict(f, i), dict(f64=cf, i32=ci), K.contact_dict(qf, qi), dict(f64=kf, i32=ki)

    # -- walls: barrier contact at the track's edges (lpvmpc_race_walls / _read, lpvmpc_wall_step_batch; walls.py) ------------------
    def race_walls(self, cfg=None, detach=False):
        """Attach the walls from the next tick on (lpvmpc_race_walls): ``cfg`` a ``walls.wall_config(...)`` result, a dict of its words,
        or None for the defaults.  Needs a race started with ``plant_params`` / ``tyre_params``; independent of heats, interactions and
        disturbances.  Attaching again replaces the binding (counters start anew); ``detach=True`` detaches."""
        from . import walls as W
        self._race_B("race_walls")
        _race_attach(self, self._lib.lpvmpc_race_walls, None if detach else W.as_config(cfg))

    def race_walls_read(self):
        """Synchronise and return the walls' outputs (lpvmpc_race_walls_read): a dict of [B] arrays named as _ffi.WALL_F64_NAMES /
        WALL_I32_NAMES (depth, impulse, impulse_total, max_impulse; hit, side, corner, hit_ticks, first_hit_tick, outside) and the
        planes f64 [4, B] / i32 [6, B]."""
        from . import walls as W
        B = self._race_B("race_walls_read")
        return W.walls_dict(*_read_planes(self, self._lib.lpvmpc_race_walls_read, B, _ffi.WALL_F64, _ffi.WALL_I32))

    def wall_step(self, plant, plant_params, t, cfg=None, nstep=None, carry=None, half_width=0.3):
        """One tick of the walls' kernel on the caller's data (lpvmpc_wall_step_batch): ``plant`` [B, 8], ``plant_params`` [B, 7] (m and
        Iz are read), ``t`` the tick number, ``cfg`` as ``race_walls``, ``nstep`` [B] the simulator steps of this tick (None: every
        vehicle steps; 0: frozen), ``carry`` the state returned by the previous call (None: ``walls.new_carry(B)``), ``half_width`` the
        track's (ignored when tracks are bound to the engine: each vehicle's palette entry has its own).  Returns (plant [B, 8] after
        the tick, outputs dict, carry)."""
        from . import walls as W
        plant, B, rows = _step_plant("wall_step", plant, plant_params)
        c = W.as_config(cfg)
        ns = _step_nstep("wall_step", nstep, B)
        k = W.new_carry(B) if carry is None else carry
        cf, ci = _carry_in("wall_step", k, _ffi.WALL_CARRY_F64, _ffi.WALL_CARRY_I32, B)
        f = np.empty((_ffi.WALL_F64, B)); i = np.empty((_ffi.WALL_I32, B), np.int32)
        self._chk(self._lib.lpvmpc_wall_step_batch(self._h, B, C.byref(c), float(half_width), int(t), ptr(plant), ptr(rows), ptr(ns), ptr(cf),
                                                   ptr(ci), ptr(f), ptr(i)))
        return plant, W.walls_dict(f, i), dict(f64=cf, i32=ci)

    # -- race event log: an ordered device-side record of what happened (lpvmpc_race_events / _read, lpvmpc_event_step_batch; events.py) --
    def race_events(self, cfg=None, detach=False):
        """Attach the event log from the next tick on (lpvmpc_race_events): ``cfg`` an ``events.event_config(...)`` result, a dict of
        its arguments (capacity, kinds), or None for the defaults (65536 events, every kind).  Attaching again replaces the binding
        and its count starts at 0; ``detach=True`` detaches.  Independent of heats, interactions, contact model and walls, in any
        order: it only observes, and it meets a heats or walls attachment at "first sight" (no event from that source on that tick)."""
        from . import events as E
        self._race_B("race_events")
        _race_attach(self, self._lib.lpvmpc_race_events, None if detach else E.as_config(cfg))

    def race_events_read(self, n=None):
        """Synchronise and return the last ``n`` kept events, oldest first (lpvmpc_race_events_read; None: all that are kept): a dict
        with ``events`` (an ``events.events_table``), ``total`` (events since the attach), ``kept`` (= min(total, capacity)) and the
        per-vehicle planes ``count`` / ``count_total`` [B] (``i32`` [2, B])."""
        from . import events as E
        B = self._race_B("race_events_read")
        if n is not None and int(n) < 0:
            raise ValueError("race_events_read: n = %r must be >= 0" % (n,))
        total = C.c_int64(0); kept = _ffi._i(0)
        out = np.zeros((_ffi.EVENT_OUT_I32, B), np.int32)
        self._chk(self._lib.lpvmpc_race_events_read(self._h, 0, C.byref(total), C.byref(kept), None, None, ptr(out)))
        m = kept.value if n is None else min(int(n), kept.value)
        i = np.empty((m, _ffi.EVENT_I32), np.int32); f = np.empty((m, _ffi.EVENT_F64))
        if m:                                   # (no tick runs between the two calls: both synchronise the engine's stream)
            self._chk(self._lib.lpvmpc_race_events_read(self._h, m, C.byref(total), C.byref(kept), ptr(i), ptr(f), None))
        return dict(events=E.events_table(i, f), total=int(total.value), kept=int(kept.value), count=out[0], count_total=out[1], i32=out)

    def event_step(self, t, phase, lap, lap_value, heats=None, heat=None, walls=None, kinds=None, carry=None, max_events=None, n_heats=None):
        """One tick of the log's device function on the caller's data (lpvmpc_event_step_batch): ``t`` the tick number, ``phase`` /
        ``lap`` [B] the race's rows after the tick, ``lap_value`` [B] the V0 of a LAP event; ``heats`` the heats' two output planes
        (a dict with ``f64`` [5, B] / ``i32`` [10, B], as ``race_standings`` / ``heat_step`` return; None: no heats) with ``heat`` [B]
        the heat of each vehicle; ``walls`` the walls' planes alike (None: no walls); ``kinds`` as ``events.kinds_mask``; ``carry`` the
        state returned by the previous call (None: ``events.new_carry(B)``, just attached); ``max_events`` the rows of the returned
        table at most (None: as many as a tick can produce).  Returns (table of this tick's events in order, cut to ``max_events``;
        n_events the tick produced; the planes dict with count / count_total; the new carry)."""
        from . import events as E
        ph = np.ascontiguousarray(np.asarray(phase).reshape(-1), np.int32)
        B = ph.shape[0]
        lp = np.ascontiguousarray(np.asarray(lap).reshape(-1), np.int32)
        lv = f64(np.broadcast_to(np.asarray(lap_value, float), (B,)), (B,), "lap_value")
        if lp.shape[0] != B:
            raise ValueError("event_step: phase and lap must have one entry per vehicle (%d)" % B)
        mask = E.kinds_mask(kinds)
        if (heats is None) != (heat is None):
            raise ValueError("event_step: heats (the two planes) and heat (the heat of each vehicle) come together")
        hf = hi = h = wf = wi = None
        nh = 0
        if heats is not None:
            from . import heats as H
            h = H.check_heats(heat, B)
            nh = int(h.max()) + 1 if n_heats is None else int(n_heats)
            hf = f64(heats["f64"], (_ffi.HEAT_F64, B), "heats f64")
            hi = np.ascontiguousarray(heats["i32"], np.int32)
            if hi.shape != (_ffi.HEAT_I32, B):
                raise ValueError("event_step: heats i32 has shape %s, expected %s" % (hi.shape, (_ffi.HEAT_I32, B)))
        if walls is not None:
            wf = f64(walls["f64"], (_ffi.WALL_F64, B), "walls f64")
            wi = np.ascontiguousarray(walls["i32"], np.int32)
            if wi.shape != (_ffi.WALL_I32, B):
                raise ValueError("event_step: walls i32 has shape %s, expected %s" % (wi.shape, (_ffi.WALL_I32, B)))
        c = E.new_carry(B) if carry is None else carry
        cf, ci = _carry_in("event_step", c, _ffi.EVENT_CARRY_F64, _ffi.EVENT_CARRY_I32, B)
        total = C.c_int64(int(c.get("total", 0)))
        if max_events is None:                   # LAP, FINISH or LOST, a PASS per other member, one contact and one wall event
            max_events = B * 4 + (int(np.sum(np.bincount(h[h >= 0]) ** 2)) if h is not None and (h >= 0).any() else 0)
        M = int(max_events)
        if M < 0:
            raise ValueError("event_step: max_events = %r must be >= 0" % (max_events,))
        ei = np.empty((M, _ffi.EVENT_I32), np.int32); ef = np.empty((M, _ffi.EVENT_F64))
        n = _ffi._i(0)
        out = np.empty((_ffi.EVENT_OUT_I32, B), np.int32)
        self._chk(self._lib.lpvmpc_event_step_batch(self._h, B, int(t), ptr(ph), ptr(lp), ptr(lv), nh, ptr(h), ptr(hf), ptr(hi), ptr(wf), ptr(wi),
                                                    mask, ptr(cf), ptr(ci), C.byref(total), M, ptr(ei), ptr(ef), C.byref(n), ptr(out)))
        m = min(M, n.value)
        return (E.events_table(ei[:m], ef[:m]), int(n.value), dict(count=out[0], count_total=out[1], i32=out),
                dict(f64=cf, i32=ci, total=int(total.value)))

    # -- device-pointer entry point (torch tensors or raw integers) -----------------------------------
    def solve_dev(self, B, x0, u_prev, vel_ref, curv_s, u_old, max_ey, xPred, uPred, status=None, iters=None,
                  resid=None, polish=None, cf_new=60.0, lap=1, stream=0):
        """Enqueue the fused tick on ``stream`` with DEVICE pointers (ints or objects with ``data_ptr()``)."""
        def dp(t):
            if t is None:
                return None
            return C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else int(t))
        self._chk(self._lib.lpvmpc_solve_batch_dev(self._h, int(B), dp(x0), dp(u_prev), dp(vel_ref), dp(curv_s),
                                                   dp(u_old), dp(max_ey), float(cf_new), int(lap), dp(xPred),
                                                   dp(uPred), dp(status), dp(iters), dp(resid), dp(polish),
                                                   C.c_void_p(int(stream))))


def observer_design_config(lim_ls, lim_hs, Qo=None, Ro=None):
    """An ``lpvmpc_observer_design``: the two limit tables [6,2] and the weights (None: the library's defaults)."""
    d = _ffi.default_observer_design()
    d.lim_ls[:] = f64(lim_ls, (6, 2), "lim_ls").ravel().tolist()
    d.lim_hs[:] = f64(lim_hs, (6, 2), "lim_hs").ravel().tolist()
    if Qo is not None:
        d.Qo[:] = f64(Qo, (6, 6), "Qo").ravel().tolist()
    if Ro is not None:
        d.Ro[:] = f64(Ro, (5, 5), "Ro").ravel().tolist()
    return d


def _delay_array(v, B, name):
    """Per-vehicle delays in simulator steps: None, or exactly B integers."""
    if v is None:
        return None
    a = np.asarray(v)
    if a.ndim != 1 or a.shape[0] != B:
        raise ValueError("%s must have %d entries (one per vehicle), got shape %s" % (name, B, a.shape))
    if not np.all(a == np.round(a)):
        raise ValueError("%s must be integer steps" % name)
    return np.ascontiguousarray(a, np.int32)


def _is_nominal(v):
    return isinstance(v, str) and v == "nominal"


def _plant_rows(v, B):
    """Per-vehicle plant rows: None (the nominal rows, chosen by the library), or exactly [B, 7] finite words."""
    if v is None:
        return None
    from .plant import check_plant_params
    return check_plant_params(v, B)


# -- what the race's attachments share (heats, interactions, contact model, walls, event log): attach / detach, read, and the step forms' inputs --
def _race_attach(solver, call, cfg):
    """Attach the checked configuration ``cfg`` through the C call, or detach (None)."""
    solver._chk(call(solver._h, None if cfg is None else C.byref(cfg)))


def _read_planes(solver, call, B, wf, wi, *more):
    """Read a layer's output planes f64 [wf, B] / i32 [wi, B] through the C call (``more``: further arrays it fills)."""
    f = np.empty((wf, B)); i = np.empty((wi, B), np.int32)
    solver._chk(call(solver._h, ptr(f), ptr(i), *[ptr(m) for m in more]))
    return f, i


def _step_plant(who, plant, plant_params):
    """A step form's plant [B, 8], copied, its B and the plant rows [B, 7]."""
    plant = f64(plant).copy()
    if plant.ndim != 2 or plant.shape[1] != 8:
        raise ValueError("%s: plant must be [B, 8], got %s" % (who, plant.shape,))
    B = plant.shape[0]
    return plant, B, f64(plant_params, (B, _ffi.PLANT_WORDS), "plant_params")


def _step_nstep(who, nstep, B):
    """A step form's simulator steps per vehicle: None, or [B] integers."""
    ns = None if nstep is None else np.ascontiguousarray(np.asarray(nstep).reshape(-1), np.int32)
    if ns is not None and ns.shape[0] != B:
        raise ValueError("%s: nstep must have one entry per vehicle (%d)" % (who, B))
    return ns


def _carry_in(who, carry, wf, wi, B, label="carry"):
    """Copies of a carried state's planes f64 [wf, B] / i32 [wi, B], shape-checked."""
    cf = f64(carry["f64"], (wf, B), label + " f64").copy()
    ci = np.ascontiguousarray(carry["i32"], np.int32).copy()
    if ci.shape != (wi, B):
        raise ValueError("%s: %s i32 has shape %s, expected %s" % (who, label, ci.shape, (wi, B)))
    return cf, ci


def _heats_args(heat, B, n_heats, half_length, half_width):
    """The heats' arguments of a C call: the checked footprint, ``heat`` [B] and the number of heats (None: the largest index + 1)."""
    from . import heats as H
    cfg = _ffi.HeatsConfig(*H.check_extents(half_length, half_width))
    h = H.check_heats(heat, B)
    return cfg, h, int(h.max()) + 1 if n_heats is None else int(n_heats)


def _tyre_rows(v, B):
    """Per-vehicle tyre rows: "pacejka" (the launch file's tyre for every vehicle), "linear" (None: the library's kind 0 rows), or
    exactly [B, 4] checked words."""
    from .plant import check_tyre_params, tyre_params
    if isinstance(v, str):
        if v not in ("pacejka", "linear"):
            raise ValueError("tyre_params must be [B, 4] rows, \"pacejka\" or \"linear\", got %r" % (v,))
        return tyre_params(B) if v == "pacejka" else None
    return check_tyre_params(v, B)


def _actuator_cfg(a):
    if not isinstance(a, _ffi.ActuatorConfig):
        raise TypeError("actuator must be an actuator.actuator_config(...) result or an _ffi.ActuatorConfig")
    return a


def handoff_operators(N, dt, cfg=None):
    """Host-only: the hand-off operators for an N-sample planner horizon at period dt (no device needed).
    Returns (W, FW), each (M, N): refs = W @ signal for x, y, yaw, vx and FW @ curvature (PMAIN:257-280)."""
    lib = _ffi.load()
    cfg = cfg if cfg is not None else _ffi.default_handoff_config()
    M = lib.lpvmpc_handoff_length(int(N), float(dt), C.byref(cfg))
    _ffi.check(None, min(M, 0))
    W = np.empty((M, int(N))); FW = np.empty((M, int(N)))
    _ffi.check(None, min(lib.lpvmpc_handoff_operators(int(N), float(dt), C.byref(cfg), ptr(W), ptr(FW)), 0))
    return W, FW


# =====================================================================================================
# drop-in classes
# =====================================================================================================
def _stack_list(L, shape, name):
    a = np.stack([np.asarray(m, dtype=np.float64) for m in L])
    if a.shape != shape:
        raise ValueError("%s has shape %s, expected %s" % (name, a.shape, shape))
    return a


class _DropInBase(object):
    # ---- the assembled QP, as the reference leaves it on the object (CTRL:79,108-110; PLAN:108) -----------------------------
    # The device path never forms these matrices; they are built on the host (qp_matrices.py) from the data of the last
    # solve() the first time one of them is read, and dropped by the next solve().
    _qp_cache = None
    _qp_inputs = None

    def _qp(self):
        if self._qp_cache is None:
            if self._qp_inputs is None:
                raise AttributeError("the QP matrices exist after the first solve()")
            self._qp_cache = self._assemble_qp(**self._qp_inputs)
        return self._qp_cache

    def qp_matrices(self):
        """(P, q, A, l, u) of the last solve in the form the reference hands to OSQP (CTRL:303-308: inequality rows first;
        PLAN:200-202: equality rows first), dense float64."""
        m = self._qp()
        return m["P"], m["q"], m["A"], m["l"], m["u"]

    E = property(lambda self: self._qp()["E"])
    L = property(lambda self: self._qp()["L"])
    Eu = property(lambda self: self._qp()["Eu"])
    q = property(lambda self: self._qp()["q"])

    def _finish(self, out, start):
        nx, N = self.n_states, self.N
        self.status_val = int(out["status"][0])
        self.status = STATUS_TEXT.get(self.status_val, "?")
        self.iters = int(out["iters"][0])
        self.status_polish = int(out["polish"][0])
        # reference: SOLVED / SOLVED_INACCURATE / MAX_ITER_REACHED count as feasible (CTRL:322-324, PLAN:214-216)
        self.feasible = 1 if self.status_val in (1, 2, -2) else 0
        if self.status_val != 1 and self.verbose_status:
            print("OSQP exited with status '%s'" % self.status)
        if self.feasible == 0:
            print("QUIT...")
        xPred = out["xPred"][0].copy()
        self.xPred = xPred
        self.uPred = out["uPred"][0].copy()
        self.LinPoints = np.concatenate((xPred[1:, :], xPred[-1:, :]), axis=0)
        self.solverTime = datetime.datetime.now() - start


class PathFollowingLPV_MPC(_DropInBase):
    """Drop-in for the reference class of the same name (CTRL:30-258).

    Same constructor arguments; ``params`` (vehicle parameters dict) and ``device`` are optional extras for
    use without ROS.  ``Solver`` is accepted for signature compatibility: the solve always runs the HIP
    ADMM path (the reference's mains only ever pass "OSQP", controllerMain.py:142,150).
    ``steeringDelay`` > 0 adds the pinned-steering equality rows of CTRL:518-527 (``OldSteering`` then has 1 + delay
    entries, CTRL:71); ``velocityDelay`` is stored and, as in the reference, never used."""

    def __init__(self, Q, R, dR, N, vt, dt, map, Solver="OSQP", steeringDelay=0, velocityDelay=0,
                 params=None, device=0, **settings):
        p = _vehicle_params(params, need_min_vel=False)
        self.lf, self.lr, self.m, self.I = p["lf"], p["lr"], p["m"], p["Iz"]
        self.Cf, self.Cr, self.mu, self.g = p["Cf"], p["Cr"], p["mu"], 9.81
        self.max_vel = p["max_vel"]
        self.A, self.B, self.C = [], [], []
        self.N = int(N)
        self.n = self.n_states = np.asarray(Q).shape[0]
        self.d = np.asarray(R).shape[0]
        self.vt = vt
        self.Q, self.R, self.dR = np.asarray(Q, float), np.asarray(R, float), np.asarray(dR, float)
        self.LinPoints = np.zeros((self.N + 2, self.n))
        self.dt = dt
        self.map = map
        self.halfWidth = map.halfWidth
        self.first_it = 1
        self.steeringDelay = steeringDelay
        self.velocityDelay = velocityDelay
        self.OldSteering = [0.0] * int(1 + steeringDelay)
        self.OldAccelera = [0.0] * int(1)
        self.OldPredicted = [0.0] * int(1 + steeringDelay + N)
        self.Solver = Solver
        self.verbose_status = True
        self._eng = BatchedSolver("controller", N, dt, self.Q, self.R, self.dR, track=map.PointAndTangent,
                                  params=p, device=device, steering_delay=int(steeringDelay), **settings)
        # one vehicle per handle: the latency form of the N = 20 kernel (four wavefronts per instance; lpvmpc.h, kernel_variant 9 --
        # other horizons and steeringDelay > 0 take their default kernels under it)
        self._eng.set_option("kernel_variant", 9)

    # CTRL:108-110 leaves G, E, L, Eu, M, q on the object; F, b exist from the constructor on (CTRL:79)
    G = property(lambda self: self._qp()["G"])
    M = property(lambda self: self._qp()["M"])

    def _bounds(self):
        c = self._eng.cfg
        return dict(vx_min=c.ctrl_vx_min, delta_max=c.ctrl_delta_max, a_max=c.ctrl_a_max, a_min_abs=c.ctrl_a_min_abs)

    @property
    def F(self):
        return self._Fb()[0]

    @property
    def b(self):
        return self._Fb()[1]

    def _Fb(self):
        if getattr(self, "_Fb_cache", None) is None:
            from . import qp_matrices
            self._Fb_cache = qp_matrices.controller_inequalities(self.N, self.n, self.d, self.max_vel, **self._bounds())
        return self._Fb_cache

    def _assemble_qp(self, **kw):
        from . import qp_matrices
        return qp_matrices.controller_qp(self.Q, self.R, self.dR, self.N, self.A, self.B, self.C, max_vel=self.max_vel,
                                         bounds=self._bounds(), **kw)

    def solve(self, x0, Last_xPredicted, uPred, NN_LPV_MPC, vel_ref, A_L, B_L, C_L, first_it):
        """CTRL:89-162.  Results in .xPred (N+1,6), .uPred (N,2), .LinPoints; returns None."""
        start = datetime.datetime.now()
        N = self.N
        uPred = np.asarray(uPred, dtype=np.float64)
        if (NN_LPV_MPC == False) and (first_it < 10):                    # noqa: E712  (CTRL:99-100)
            xl = np.asarray(Last_xPredicted, dtype=np.float64)[:N, :6]
            A, Bm = self._eng.estimate_abc(xl[None], uPred[:N, 0][None])
            A, Bm = A[0], Bm[0]
        else:
            A = _stack_list(A_L, (N, 6, 6), "A_L")
            Bm = _stack_list(B_L, (N, 6, 2), "B_L")
        self.A = [A[i] for i in range(N)]
        self.B = [Bm[i] for i in range(N)]
        self.C = [np.zeros((6, 1)) for _ in range(N)]
        vr = np.asarray(vel_ref, dtype=np.float64).reshape(-1)
        vfull = np.concatenate((vr[:N], vr[-1:]))                         # CTRL:434-438: stage N tracks vel_ref[-1]
        d = int(self.steeringDelay)
        # CTRL:395 (uOld) followed by the pinned commands OldSteering[1 .. delay] of CTRL:523
        u_old = np.array([[self.OldSteering[0], self.OldAccelera[0]] + [float(v) for v in self.OldSteering[1:1 + d]]], dtype=np.float64)
        self._qp_cache = None
        self._qp_inputs = dict(x0=np.array(x0, dtype=np.float64).reshape(6), u_old=u_old[0, :2].copy(), vel_ref=vfull.copy(),
                               steer_hist=tuple(u_old[0, 2:]))
        self.linearizationTime = datetime.datetime.now() - start
        start = datetime.datetime.now()
        out = self._eng.solve_AB(np.asarray(x0, float).reshape(1, 6), A[None], Bm[None], vfull[None], u_old)
        self._finish(out, start)

    def LPVPrediction(self, x, u, vel_ref, curv_ref, Cf_new, LapNumber):
        """CTRL:166-258.  Returns (STATES_vec (N,6), Atv, Btv, Ctv) with Atv/Btv/Ctv lists of N arrays."""
        N = self.N
        vr = np.asarray(vel_ref, dtype=np.float64).reshape(-1)
        vfull = np.concatenate((vr[:N], vr[-1:]))
        curv = None
        if LapNumber != 0:
            curv = np.asarray(curv_ref, dtype=np.float64).reshape(-1)[:N][None]
        S, A, Bm = self._eng.lpv(np.asarray(x, float).reshape(1, 6), np.asarray(u, float)[:N, :2][None], vfull[None],
                                 curv, cf_new=float(Cf_new), lap=int(LapNumber))
        return (S[0], [A[0, i] for i in range(N)], [Bm[0, i] for i in range(N)],
                [np.zeros((6, 1)) for _ in range(N)])


class LPV_MPC_Planner(_DropInBase):
    """Drop-in for the reference LPV-MPP planner class (PLAN:29-320)."""

    def __init__(self, Q, R, dR, L_cf, N, dt, map, Solver="OSQP", params=None, device=0, **settings):
        p = _vehicle_params(params, need_min_vel=True)
        self.A, self.B, self.C = [], [], []
        self.N = int(N)
        self.nx = self.n_states = np.asarray(Q).shape[0]
        self.nu = np.asarray(R).shape[0]
        self.Q = np.asarray(Q, float); self.QN = self.Q
        self.R, self.dR, self.L_cf = np.asarray(R, float), np.asarray(dR, float), np.asarray(L_cf, float)
        self.LinPoints = np.zeros((self.N + 2, self.nx))
        self.dt = dt
        self.map = map
        self.halfWidth = map.halfWidth
        self.first_it = 1
        self.Solver = Solver
        self.steeringDelay = 0
        self.OldSteering = [0.0]
        self.OldAccelera = [0.0]
        self.lf, self.lr, self.m, self.I = p["lf"], p["lr"], p["m"], p["Iz"]
        self.Cf, self.Cr, self.mu, self.g, self.epss = p["Cf"], p["Cr"], p["mu"], 9.81, 0.00000001
        self.max_vel, self.min_vel = p["max_vel"], p["min_vel"]
        self.verbose_status = False                                       # PLAN:212-213: status print commented out
        self._eng = BatchedSolver("planner", N, dt, self.Q, self.R, self.dR, L_cf=self.L_cf,
                                  track=map.PointAndTangent, params=p, device=device, **settings)
        # one vehicle per handle: the latency form where a horizon has one of its own (N = 20; N = 30 / 40 take four wavefronts for a
        # lone instance by default) -- lpvmpc.h, kernel_variant 9
        self._eng.set_option("kernel_variant", 9)

    Aeq = property(lambda self: self._qp()["Aeq"])                      # PLAN:108

    def _assemble_qp(self, **kw):
        from . import qp_matrices
        c = self._eng.cfg
        xlo, xhi = np.array(c.plan_xmin[:]), np.array(c.plan_xmax[:])
        xlo[0], xhi[0] = self.min_vel, self.max_vel                       # PLAN:176-177
        xlo[3], xhi[3] = -kw["max_ey"], kw["max_ey"]
        return qp_matrices.planner_qp(self.Q, self.R, self.dR, self.L_cf, self.N, self.A, self.B, self.C, min_vel=self.min_vel,
                                      max_vel=self.max_vel, xbox=(xlo, xhi), ubox=(np.array(c.plan_umin[:]), np.array(c.plan_umax[:])), **kw)

    def solve(self, x0, Last_xPredicted, uPred, A_LPV, B_LPV, C_LPV, first_it, max_ey):
        """PLAN:86-236."""
        start = datetime.datetime.now()
        N = self.N
        if first_it < 2:                                                  # PLAN:99-100
            xl = np.asarray(Last_xPredicted, dtype=np.float64)[:N, :6]
            delta = np.asarray(uPred, dtype=np.float64).reshape(-1)[:N] if np.ndim(uPred) < 2 or np.shape(uPred)[1] == 1 \
                else np.asarray(uPred, dtype=np.float64)[:N, 0]
            A, Bm = self._eng.estimate_abc(xl[None], delta[None])
            A, Bm = A[0], Bm[0]
        else:
            A = _stack_list(A_LPV, (N, 5, 5), "A_LPV")
            Bm = _stack_list(B_LPV, (N, 5, 2), "B_LPV")
        self.A = [A[i] for i in range(N)]
        self.B = [Bm[i] for i in range(N)]
        self.C = [np.zeros((5, 1)) for _ in range(N)]
        u_old = np.array([[self.OldSteering[0], self.OldAccelera[0]]], dtype=np.float64)   # PLAN:114 (quirk Q3)
        self._qp_cache = None
        self._qp_inputs = dict(x0=np.array(x0, dtype=np.float64).reshape(5), u_old=u_old[0].copy(), max_ey=float(max_ey))
        out = self._eng.solve_AB(np.asarray(x0, float).reshape(1, 5), A[None], Bm[None], None, u_old,
                                 max_ey=float(max_ey))
        self._finish(out, start)

    def LPVPrediction(self, x, SS, u):
        """PLAN:242-320."""
        N = self.N
        S, A, Bm = self._eng.lpv(np.asarray(x, float).reshape(1, 5), np.asarray(u, float)[:N, :2][None], None,
                                 np.asarray(SS, float).reshape(-1)[:N + 1][None])
        return (S[0], [A[0, i] for i in range(N)], [Bm[0, i] for i in range(N)],
                [np.zeros((5, 1)) for _ in range(N)])


# =====================================================================================================
# caller-side helpers of the two nodes, single vehicle
# =====================================================================================================
class PlannerHandoff(object):
    """The post-processing block of plannerMain.py for one vehicle: ``refs = PlannerHandoff(Planner).update()`` replaces
    PMAIN:112 (filter design), :189-224 (s integration, pose reconstruction) and :257-280 (resampling, filtering).

    State carried between ticks, as in the node: ``SS`` (N+1,), ``Xlast / Ylast / Thetalast``.  After ``update()``:
    ``xp, yp, yaw, vel, curv`` (N,) at the planner's rate and ``x_d, y_d, psi_d, vx_d, curv_d`` (M,) -- the five arrays
    of the My_Planning message (PMAIN:303-307).  Computed on the device through lpvmpc_handoff_batch."""

    def __init__(self, planner, handoff_config=None):
        self._eng = planner._eng
        self.N = planner.N
        self.M = self._eng.handoff_setup(handoff_config)
        self.SS = np.zeros(self.N + 1)
        self.Xlast = self.Ylast = self.Thetalast = 0.0
        self._planner = planner

    def update(self, xPred=None):
        xPred = self._planner.xPred if xPred is None else xPred
        o = self._eng.handoff(np.asarray(xPred, float)[None], self.SS[None], np.array([[self.Xlast, self.Ylast, self.Thetalast]]),
                              want_sig=True)
        self.SS = o["SS"][0]
        self.Xlast, self.Ylast, self.Thetalast = (float(v) for v in o["pose"][0])
        self.xp, self.yp, self.yaw, self.vel, self.curv = (o["sig"][0, i] for i in range(5))
        self.x_d, self.y_d, self.psi_d, self.vx_d, self.curv_d = (o["refs"][0, i] for i in range(5))
        return o["refs"][0]


def body_frame_errors(x, y, psi, xd, yd, psid, s0, vx, vy, curv, dt):
    """Body_Frame_Errors of controllerMain.py:495-506 -> (s, ex, ey, epsi); host arithmetic, a dozen flops."""
    ex = (x - xd) * np.cos(psid) + (y - yd) * np.sin(psid)
    ey = -(x - xd) * np.sin(psid) + (y - yd) * np.cos(psid)
    d = psi - psid
    epsi = 2 * np.pi + d if d < -np.pi else (d - 2 * np.pi if d > np.pi else d)            # TRACK:413-421 wrap()
    s = s0 + ((vx * np.cos(epsi) - vy * np.sin(epsi)) / (1 - ey * curv)) * dt
    return s, ex, ey, epsi


class RaceFleet(object):
    """A fleet of B vehicles running the reference's whole experiment on the device (lpvmpc_race_*): lap 0 under the
    path-following controller at 1 m/s, each vehicle's own lap event, then planner + trajectory-tracking controller until it has
    driven ``laps`` racing laps.  Three engines with the reference's tunings (CTRL_TUNINGS["path"], CTRL_TUNINGS["race"], the
    PLAN_* weights).  ``options``: race options of ``BatchedSolver.race_init`` (n_sub_lap0, n_sub, q9_swap, plan_max_ey, dt_sim,
    mu_sim) and engine settings (e.g. kernel_variant) applied to all three engines.  ``estimator``: an
    ``observer.observer_config(...)`` result runs the race with the state estimator and the simulated sensors in the loop.
    ``actuator``: an ``actuator.actuator_config(...)`` result puts the actuator delays / servo lag in the plant (per-vehicle
    delay_a / delay_df in steps); ``steering_delay``: both controllers' steeringDelay (needs ``actuator``, e.g.
    actuator.controller_delay(delay_df_s)).  ``plant_params``: [B, 7] rows (lf, lr, m, Iz, Cf, Cr, mu) give every vehicle its own
    plant (plant.sample_plant_params for a mismatch sweep), ``tyre_params`` [B, 4] rows (kind, B, C, c_f; or "pacejka") its own tyre
    (plant.tyre_params, plant.sample_tyre_params); the controllers and the planner keep the nominal, linear-tyre model unless
    ``model_params`` is given: [B, 7] rows bound to the path, tt and planner engines (BatchedSolver.set_model_params), or the string
    "plant": each vehicle's model is its plant row (the matched experiment; the nominal plant rows where plant_params is None or
    "nominal").  ``path_tunings`` / ``tt_tunings`` / ``plan_tunings``: [B, 64] tuning rows (tuning.tuning_rows, tuning.sample_tunings)
    bound to the path, tt and planner engine (BatchedSolver.set_tunings): vehicle b races with its own weights and limits.
    ``estimator_params`` (with ``estimator``): the estimator's model rows, [B, 7], "plant" (each vehicle's plant row) or "model" (the
    rows ``model_params`` binds); the gain tables are designed on the device for each row, on the estimator configuration's limit
    tables with ``estimator_design``'s weights (dict(Qo=, Ro=), default: observer_vertex_gains'), and bound to the path engine
    (BatchedSolver.set_observer_vehicles).  None: the estimator keeps its own constants and the configuration's tables.
    ``track_map``: one map, or a sequence of maps (a palette, at most 64: track.Map, track.mirrored, track.scaled, ...) with
    ``track_of`` [B], the palette entry of each vehicle: one race with vehicles on different circuits, each with its own lap length,
    half width and slack (``tracks()`` reads the binding back; ``plan_max_ey`` stays one value per race).
    ``disturbance``: [B, 13] rows (disturbance.disturbance_rows, disturbance.sample_disturbances) or dict(rows=, seed=,
    vehicle_offset=, n_bound=): gusts, a kick and grip patches on the plant from the first tick on (``disturb`` attaches or detaches
    mid-race, ``disturbance()`` reads rows and state back); it selects ``tyre_params="linear"`` when none is given.
    ``sensor_faults`` (with ``estimator``): [B, 12] rows (sensor_faults.fault_rows, sensor_faults.sample_faults) or dict(rows=, seed=,
    vehicle_offset=): GPS loss and jumps, IMU bias and drift, a slipping or stuck encoder from the first tick on (``fault`` attaches or
    detaches mid-race, ``faults()`` reads the rows back); it selects ``tyre_params="linear"`` when none is given.
    ``heats``: heat [B] (-1: none) or dict(heat=, turns0=, half_length=, half_width=): heats attached from the first tick on (``heats``
    attaches or detaches mid-race, ``standings()`` reads them).  ``interactions`` (with ``heats``): True for the defaults, an
    ``interactions.interaction_config(...)`` result or a dict of its words: slipstream and contact response between the members of a
    heat from the first tick on (``interact`` attaches or detaches mid-race, ``interactions()`` reads the outputs back); it selects
    ``tyre_params="linear"`` when none is given.  ``contact`` (with ``interactions``): True for the defaults, a
    ``contact.contact_config(...)`` result or a dict of its words: the corner form of the car-to-car contact, with friction and a yaw
    response, from the first tick on (``contact`` attaches or detaches mid-race, ``contacts()`` reads its planes back).
    ``walls``: True for the defaults, a ``walls.wall_config(...)`` result or a dict of its words: barrier contact at the track's edges
    from the first tick on (``wall`` attaches or detaches mid-race, ``walls()`` reads the outputs back); it selects
    ``tyre_params="linear"`` when none is given.
    ``events``: True for the defaults, an ``events.event_config(...)`` result or a dict of its arguments (capacity, kinds): the event
    log from the first tick on, attached last (``log`` attaches or detaches mid-race, ``events()`` reads the ordered record back)."""

    def __init__(self, track_map, plant0, laps=1, N=20, Np=40, half_track0=None, device=0, estimator=None, actuator=None,
                 steering_delay=0, delay_a=None, delay_df=None, plant_params=None, model_params=None, path_tunings=None,
                 tt_tunings=None, plan_tunings=None, tyre_params=None, estimator_params=None, estimator_design=None, track_of=None,
                 disturbance=None, sensor_faults=None, heats=None, interactions=None, walls=None, contact=None, events=None,
                 **options):
        from .workloads import CTRL_TUNINGS, PLAN_L, PLAN_Q, PLAN_R, PLAN_dR
        if interactions is not None and interactions is not False and heats is None:
            raise ValueError("interactions needs heats: the vehicles of a heat act on each other")
        if contact is not None and contact is not False and (interactions is None or interactions is False):
            raise ValueError("contact needs interactions: the contact model is a form of their contact")
        race_keys = ("n_sub_lap0", "n_sub", "q9_swap", "plan_max_ey", "dt_sim", "mu_sim")
        race_opts = {k: v for k, v in options.items() if k in race_keys}
        engine_opts = {k: v for k, v in options.items() if k not in race_keys}
        Qp, Rp, dRp = CTRL_TUNINGS["path"]; Qr, Rr, dRr = CTRL_TUNINGS["race"]
        # a sequence of maps with track_of: every vehicle on its own track (lpvmpc_set_tracks on the three engines, the start through
        # the most general entry); a single map, or a sequence of one without track_of, keeps the unbound path
        from .track import fleet_tracks
        maps, of = fleet_tracks(track_map, track_of, f64(plant0).reshape(-1, 8).shape[0])
        track_map = maps[0]
        tab = track_map.PointAndTangent
        self.map = track_map
        self.maps = maps
        sd = {"steering_delay": int(steering_delay)} if steering_delay else {}
        self.path = BatchedSolver("controller", N, 1.0 / 30.0, Qp, Rp, dRp, track=tab, device=device, **sd)
        self.tt = BatchedSolver("controller", N, 1.0 / 30.0, Qr, Rr, dRr, track=tab, device=device, **sd)
        self.planner = BatchedSolver("planner", Np, 0.05, PLAN_Q, PLAN_R, PLAN_dR, L_cf=PLAN_L, track=tab, device=device)
        for e in (self.path, self.tt, self.planner):
            for k, v in engine_opts.items():
                e.set_option(k, int(v))
        self.planner.handoff_setup()
        self.dt_sim = float(race_opts.get("dt_sim", 0.005))
        if model_params is not None:
            B = f64(plant0).reshape(-1, 8).shape[0]
            if isinstance(model_params, str):
                if model_params != "plant":
                    raise ValueError("model_params must be [B, 7] rows or \"plant\", got %r" % (model_params,))
                from .plant import plant_params as nominal_plant
                rows = (nominal_plant(B, self.path, race_opts.get("mu_sim", 0.05)) if plant_params is None or _is_nominal(plant_params)
                        else _plant_rows(plant_params, B))
            else:
                from .model import check_model_params
                rows = check_model_params(model_params, B)
            for e in (self.path, self.tt, self.planner):
                e.set_model_params(rows)
        for e, rows in ((self.path, path_tunings), (self.tt, tt_tunings), (self.planner, plan_tunings)):
            if rows is not None:
                from .tuning import check_tuning_rows
                e.set_tunings(check_tuning_rows(rows, f64(plant0).reshape(-1, 8).shape[0], e.kind))
        if estimator_params is not None:
            if estimator is None:
                raise ValueError("estimator_params needs an estimator")
            B = f64(plant0).reshape(-1, 8).shape[0]
            if isinstance(estimator_params, str):
                from .plant import plant_params as nominal_plant
                if estimator_params == "plant":
                    erows = (nominal_plant(B, self.path, race_opts.get("mu_sim", 0.05)) if plant_params is None or _is_nominal(plant_params)
                             else _plant_rows(plant_params, B))
                elif estimator_params == "model" and model_params is not None:
                    erows = self.path.model_params_read()
                else:
                    raise ValueError("estimator_params must be [B, 7] rows, \"plant\" or (with model_params) \"model\", got %r" % (estimator_params,))
            else:
                erows = _plant_rows(estimator_params, B)
            lim = np.array(estimator.lim_ls[:]).reshape(6, 2), np.array(estimator.lim_hs[:]).reshape(6, 2)
            self.path.set_observer_vehicles(erows, design=observer_design_config(lim[0], lim[1], **(estimator_design or {})))
            if plant_params is None and tyre_params is None:
                plant_params = "nominal"                         # the starts that run the binding
        if of is not None:
            for e in (self.path, self.tt, self.planner):
                e.set_tracks(maps, of)
            if tyre_params is None:
                tyre_params = "linear"                           # the start that runs the binding (each track's width and slack)
        if disturbance is not None and tyre_params is None:
            tyre_params = "linear"                               # the start whose tables the disturbances scale
        if sensor_faults is not None and tyre_params is None:
            tyre_params = "linear"                               # the start whose fused kernel has a faulted form
        if interactions is not None and interactions is not False:
            if tyre_params is None:
                tyre_params = "linear"                           # the start whose plant table holds the masses and the drag words
        if walls is not None and walls is not False and tyre_params is None:
            tyre_params = "linear"                               # the start whose plant table holds m and Iz
        self.path.race_init(self.tt, self.planner, plant0, half_track0=half_track0, laps=laps, half_width=track_map.halfWidth,
                            slack=track_map.slack, estimator=estimator, actuator=actuator, delay_a=delay_a, delay_df=delay_df,
                            plant_params=plant_params, tyre_params=tyre_params, **race_opts)
        if disturbance is not None:
            self.disturb(**disturbance) if isinstance(disturbance, dict) else self.disturb(disturbance)
        if sensor_faults is not None:
            self.fault(**sensor_faults) if isinstance(sensor_faults, dict) else self.fault(sensor_faults)
        if heats is not None:
            self.heats(**heats) if isinstance(heats, dict) else self.heats(heats)
        if interactions is not None and interactions is not False:
            self.interact(None if interactions is True else interactions)
        if contact is not None and contact is not False:
            self.contact(None if contact is True else contact)
        if walls is not None and walls is not False:
            self.wall(None if walls is True else walls)
        if events is not None and events is not False:
            self.log(None if events is True else events)

    def fault(self, rows, seed=0, vehicle_offset=0):
        """Attach sensor faults from the next tick on (BatchedSolver.set_sensor_faults on the path engine); ``None`` detaches."""
        self.path.set_sensor_faults(rows, seed=seed, vehicle_offset=vehicle_offset)

    def faults(self):
        """The attached sensor fault rows [B, 12], or None (BatchedSolver.sensor_faults)."""
        return self.path.sensor_faults()

    def disturb(self, rows, seed=0, vehicle_offset=0, n_bound=None):
        """Attach plant disturbances from the next tick on (BatchedSolver.set_disturbances on the path engine); ``None`` detaches."""
        self.path.set_disturbances(rows, seed=seed, vehicle_offset=vehicle_offset, n_bound=n_bound)

    def disturbance(self):
        """The attached disturbance rows [B, 13] and the model's state [B, 5] (BatchedSolver.disturbances_read)."""
        return self.path.disturbances_read()

    def wear(self, rows):
        """Attach tyre wear and temperature from the next tick on (BatchedSolver.set_tyre_wear on the path engine): ``rows`` [B, 12]
        (tyre_wear.tyre_wear_rows / sample_tyre_wear); ``None`` detaches.  The race must have tyre rows (``tyre_params``)."""
        self.path.set_tyre_wear(rows)

    def tyre_wear(self):
        """The attached wear rows [B, 12] and the tyre sets' state [B, 6] = (W, T, P, g, ticks, E) (BatchedSolver.tyre_wear_read)."""
        return self.path.tyre_wear_read()

    def fit_tyres(self, mask):
        """A tyre change between ticks for the vehicles of ``mask`` [B] (BatchedSolver.tyre_wear_fit)."""
        self.path.tyre_wear_fit(mask)

    def run(self, n_ticks):
        """Enqueue n_ticks controller ticks (no synchronisation)."""
        self.path.race_tick(n_ticks)

    def state(self):
        return self.path.race_read()

    def estimate(self):
        """The estimator's state of a race started with ``estimator``: estimate [B,6] = [vx vy psiDot x y yaw] and the latest
        sensor reading [B,5] = [vx psiDot x y yaw]."""
        return self.path.observer_read()

    def actuator(self):
        """Of a race started with ``actuator``: act_state and the path / tt controllers' u_old histories (BatchedSolver.actuator_read)."""
        return self.path.actuator_read()

    def plant_params(self):
        """The vehicles' plant rows [B, 7] of a race started with ``plant_params`` (BatchedSolver.plant_params_read)."""
        return self.path.plant_params_read()

    def tyre_params(self):
        """The vehicles' tyre rows [B, 4] of a race started with ``tyre_params`` (BatchedSolver.tyre_params_read)."""
        return self.path.tyre_params_read()

    def model_params(self):
        """The model rows [B, 7] bound to the race's three engines by ``model_params`` (read from the path engine), or None."""
        return self.path.model_params_read()

    def tracks(self):
        """The tracks bound to the race's three engines by a sequence ``track_map`` with ``track_of`` (BatchedSolver.tracks_read on the
        path engine), or None for a race on a single map."""
        return self.path.tracks_read()

    def tunings(self):
        """The tuning rows bound to the (path, tt, planner) engines, each [B, 64] or None."""
        return self.path.tunings_read(), self.tt.tunings_read(), self.planner.tunings_read()

    def lap_times(self):
        """[B, laps+1] simulated seconds of lap 0, 1, ..., laps (NaN where the lap has not been completed)."""
        ls, _ = self.path.race_laps()
        d = (ls[:, 1:] - ls[:, :-1]).astype(float) * self.dt_sim
        d[(ls[:, 1:] < 0) | (ls[:, :-1] < 0)] = np.nan
        return d

    def record(self, capacity, stride=1):
        """Record the race from the next tick on (BatchedSolver.race_record): the last ``capacity`` records, one every ``stride``
        ticks, and the per-lap statistics of every tick.  ``record(0)`` stops recording."""
        self.path.race_record(capacity, stride)

    def trace(self, last=None):
        """The kept records, oldest first (BatchedSolver.race_record_read)."""
        return self.path.race_record_read(last)

    def lap_stats(self):
        """Per-lap statistics of the recorded ticks (BatchedSolver.race_lap_stats) with rmse_v / rmse_ey / rmse_epsi [B, laps+1]
        (RMSE_ve / RMSE_ye / RMSE_thetae of CMAIN:101-106; NaN where the lap has no counted tick)."""
        from .telemetry import add_rmse
        return add_rmse(self.path.race_lap_stats())

    def heats(self, heat, turns0=None, half_length=0.4, half_width=0.2):
        """Attach heats from the next tick on (BatchedSolver.race_heats): ``heat`` [B], the heat of each vehicle (-1: none); the
        device then keeps each heat's order, gaps, passes, line crossings and footprint clearances.  ``heats(None)`` detaches."""
        self.path.race_heats(heat, turns0=turns0, half_length=half_length, half_width=half_width)

    def standings(self):
        """The standings of the attached heats (BatchedSolver.race_standings); ``telemetry.standings_table`` prints them."""
        return self.path.race_standings()

    def interact(self, cfg=None, detach=False):
        """Attach the interactions from the next tick on (BatchedSolver.race_interactions): slipstream and contact response between the
        members of the attached heats.  ``cfg``: None (the defaults), a dict of words or an ``interactions.interaction_config(...)``
        result; ``interact(detach=True)`` detaches.  ``heats(...)`` detaches them too."""
        self.path.race_interactions(cfg, detach=detach)

    def interactions(self):
        """The outputs of the attached interactions (BatchedSolver.race_interactions_read): shelter, live mu, impulses, leader, hits."""
        return self.path.race_interactions_read()

    def contact(self, cfg=None, detach=False):
        """Attach the contact model on top of the interactions from the next tick on (BatchedSolver.race_contact): ``cfg`` None (the
        defaults), a dict of words or a ``contact.contact_config(...)`` result; ``contact(detach=True)`` goes back to the centres form.
        ``interact(...)`` and ``heats(...)`` detach it too."""
        self.path.race_contact(cfg, detach=detach)

    def contacts(self):
        """The planes of the attached contact model (BatchedSolver.race_contact_read): friction impulse, yaw kicks, partners."""
        return self.path.race_contact_read()

    def wall(self, cfg=None, detach=False):
        """Attach the walls from the next tick on (BatchedSolver.race_walls): ``cfg`` None (the defaults), a dict of words or a
        ``walls.wall_config(...)`` result; ``wall(detach=True)`` detaches."""
        self.path.race_walls(cfg, detach=detach)

    def walls(self):
        """The outputs of the attached walls (BatchedSolver.race_walls_read): depth, impulses, hit, side, corner, counters, outside."""
        return self.path.race_walls_read()

    def log(self, cfg=None, detach=False):
        """Attach the event log from the next tick on (BatchedSolver.race_events): ``cfg`` None (the defaults), a dict of arguments
        or an ``events.event_config(...)`` result; ``log(detach=True)`` detaches."""
        self.path.race_events(cfg, detach=detach)

    def events(self, n=None):
        """The last ``n`` kept events of the attached log, oldest first, in the log's order (tick, vehicle, kind, other), and the
        count of every event since the attach: (``events.events_table``, total) (BatchedSolver.race_events_read)."""
        r = self.path.race_events_read(n)
        return r["events"], r["total"]

    def snapshot(self):
        """The race's whole per-vehicle state and tick counter (BatchedSolver.race_snapshot): a ``snapshot.RaceSnapshot`` with
        ``to_bytes`` / ``save`` for a checkpoint.  State only: a race restored elsewhere is first built with the same arguments."""
        return self.path.race_snapshot()

    def restore(self, snap):
        """Continue from a snapshot of this race or of one built alike (BatchedSolver.race_restore): rewind, or resume a checkpoint."""
        self.path.race_restore(snap)

    def clone(self, src):
        """Vehicle b takes the state of vehicle src[b] and keeps its own bindings (BatchedSolver.race_clone); returns the number moved.
        Sensor noise and gusts are keyed by the vehicle's slot, so a clone draws its own future."""
        return self.path.race_clone(src)

    def respawn(self, seed):
        """Fill every lost slot (non-finite plant) with a clone of a vehicle that is still driving, on a track-bound race one of the
        slot's own track, chosen by ``numpy.random.default_rng(seed)`` (snapshot.respawn_sources): importance splitting's
        resampling step.  Finished vehicles are frozen, not lost, and are neither filled nor cloned.  Returns the ``src`` map; any
        weights of a splitting estimator are the caller's to keep."""
        from .snapshot import respawn_sources
        st = self.path.race_read()
        finite = np.isfinite(st["plant"]).all(axis=1)
        tr = self.tracks()
        src = respawn_sources(finite & (st["phase"] < 2), None if tr is None else tr["track_of"], seed, lost=~finite)
        if (src != np.arange(src.shape[0])).any():
            self.path.race_clone(src)
        return src

    def close(self):
        for e in (self.path, self.tt, self.planner):
            e.close()
