"""Host replay of the race engine (lpvmpc_race_*), composed of the oracle pieces: lap 0 and the event tick with
oracle/lpv_ref.py (seed trajectories, ABC linearisation, LPV roll-out, QP) + the OSQP restatement + oracle/plant_ref.py, then one
oracle.cascade_ref.CascadeRef (B = 1) per vehicle from the state it has after its event tick.  The schedule is
ControllerNode.step / PlannerNode.step (ros_nodes.py) with the engine's definitions: the first 9 ticks of the race are seed
ticks, a vehicle finishing its laps is frozen, a vehicle entering a tick with a non-finite plant is lost.  Not replayed: a lap event inside the 9 seed ticks."""
from __future__ import annotations

import numpy as np

from oracle import cascade_ref as CR, lpv_ref as L, osqp_ref, plant_ref as PR


class RaceRef:
    def __init__(self, track, plant0, half_track0=None, laps=1, N=20, dt=1.0 / 30, half_width=0.2, slack=0.15, plan_max_ey=0.2,
                 n_sub_lap0=7, n_sub=(7, 7, 6), params=None):
        """``params``: the vehicle (DEFAULT_PARAMS updated by it) of the lap-0 and event ticks' LPV, QP and plant steps.  The
        racing ticks (CascadeRef) know the default vehicle only: a vehicle of another kind reaching its lap event raises."""
        from lpvmpc import workloads as W
        self.p = dict(L.DEFAULT_PARAMS, **(params or {}))
        self.sim_p = dict(PR.SIM_PARAMS, **{k: self.p[k] for k in ("lf", "lr", "m", "Iz")})
        self.track = np.asarray(track, float)
        self.TL = float(self.track[-1, 3] + self.track[-1, 4])
        self.plant = np.array(plant0, float).reshape(-1, 8)
        self.B = self.plant.shape[0]
        self.half = np.zeros(self.B, int) if half_track0 is None else np.broadcast_to(np.asarray(half_track0, int), (self.B,)).copy()
        self.laps, self.N, self.dt, self.hw, self.slack, self.max_ey = laps, N, dt, half_width, slack, plan_max_ey
        self.n_sub_lap0, self.n_sub = n_sub_lap0, tuple(n_sub)
        self.path_tuning, self.tt_tuning = W.CTRL_TUNINGS["path"], W.CTRL_TUNINGS["race"]
        self.plan_weights = (W.PLAN_Q, W.PLAN_R, W.PLAN_dR, W.PLAN_L)
        self.phase = np.zeros(self.B, int)
        self.lap = np.zeros(self.B, int)
        self.cmd = np.zeros((self.B, 2))
        self.uPred_path = np.zeros((self.B, N, 2))
        self.local = np.zeros((self.B, 6))
        self.iters = np.zeros(self.B, int)
        self.status = np.zeros(self.B, int)
        self.casc = [None] * self.B
        self.event_tick = np.full(self.B, -1)
        self.t = 0

    def _solve_path(self, b, x_meas, seed):
        p, N = self.p, self.N
        Q, R, dR = self.path_tuning
        if seed:
            xx, uu = L.ctrl_seed_vectors(x_meas)
            A, Bm = L.ctrl_estimate_abc(p, self.dt, N, self.track, xx[:N], uu[:N])
            x0 = x_meas
        else:
            S, A, Bm = L.ctrl_lpv_prediction(p, self.dt, N, self.track, x_meas, self.uPred_path[b], np.ones(N + 1), np.zeros(N), 60.0, 0)
            x0 = S[0]
        qp = L.ctrl_build_qp(Q, R, dR, N, A, Bm, x0, self.cmd[b], np.ones(N + 1), p["max_vel"])
        r = osqp_ref.solve_qp(qp.P, qp.q, qp.A, qp.l, qp.u)
        _x, u, _ = L.unpack_solution(r.x, 6, 2, N)
        return u, r.info.iter, r.info.status_val

    def _solve_tt_event(self, b, x_meas):
        p, N = self.p, self.N
        Q, R, dR = self.tt_tuning
        S, A, Bm = L.ctrl_lpv_prediction(p, self.dt, N, self.track, x_meas, self.uPred_path[b], np.ones(N + 1), np.zeros(N), 60.0, 1)
        qp = L.ctrl_build_qp(Q, R, dR, N, A, Bm, x_meas, self.cmd[b], np.ones(N + 1), p["max_vel"])
        r = osqp_ref.solve_qp(qp.P, qp.q, qp.A, qp.l, qp.u)
        _x, u, _ = L.unpack_solution(r.x, 6, 2, N)
        return u, r.info.iter, r.info.status_val

    def tick(self):
        seed = self.t < 9
        for b in range(self.B):
            if self.phase[b] >= 2:
                self.iters[b] = 0
                continue
            if not np.all(np.isfinite(self.plant[b])):
                self.phase[b] = 3; self.iters[b] = 0
                continue
            if self.phase[b] == 1:
                c = self.casc[b]
                lap_before = c.lap[0]
                c.tick()                                            # measure, solve, plant (the lap event is inside measure)
                if c.lap[0] != lap_before and c.lap[0] > self.laps:
                    # finishing tick: frozen before anything of this tick is applied -- undo the replayed tick
                    self.phase[b] = 2; self.lap[b] = c.lap[0]; self.iters[b] = 0
                    continue
                self.plant[b] = c.plant[0]; self.cmd[b] = c.cmd[0]; self.local[b] = c.local[0]; self.lap[b] = c.lap[0]
                self.iters[b] = c.ctrl["iters"][0]; self.status[b] = c.ctrl["status"][0]
                continue
            st = self.plant[b]
            s, ey, epsi, _ = PR.get_local_position(self.track, self.hw, self.slack, st[0], st[1], st[6])
            Lc = np.array([st[2] if st[2] >= 0.01 else 0.01, st[3], st[7], ey, s, epsi])     # CMAIN:183-188 (quirk Q9)
            self.local[b] = Lc
            if s >= 3 * self.TL / 4:
                self.half[b] = 1
            event = self.half[b] == 1 and s <= self.TL / 4
            if event and self.p != L.DEFAULT_PARAMS:
                raise NotImplementedError("RaceRef: the racing ticks (CascadeRef) replay the default vehicle only")
            if event and not seed:
                u, it, stt = self._solve_tt_event(b, Lc)
            else:
                u, it, stt = self._solve_path(b, Lc, seed)
                self.uPred_path[b] = u
            self.iters[b], self.status[b] = it, stt
            self.cmd[b] = u[0]
            for _ in range(self.n_sub_lap0):
                st = PR.simulator_f(st, [self.cmd[b, 1], self.cmd[b, 0]], self.sim_p)
            self.plant[b] = st
            if event:
                self.half[b] = 0; self.lap[b] = 1; self.phase[b] = 1; self.event_tick[b] = self.t
                self.casc[b] = CR.CascadeRef(self.track, self.tt_tuning, self.plan_weights, st[None], self.cmd[b][None], u[None], lap0=1,
                                             half_width=self.hw, slack=self.slack, plan_max_ey=self.max_ey, n_sub=self.n_sub)
        self.t += 1
