"""tests/_race_ref.py RaceRef with per-vehicle weights: vehicle b's lap-0 and event solves and the CascadeRef it races with take
path_weights[b] / tt_weights[b] = (Q, R, dR) and plan_weights[b] = (Q, R, dR, L_cf) (the weight words of the rows bound with
lpvmpc_set_tunings; the oracle pieces RaceRef is composed of take no other limits).  RaceRef reads its three tunings as
attributes inside the loop over the vehicles, after the vehicle's solve of the tick: here they are properties that answer for
the vehicle being solved.  With the nominal weights for every vehicle it is RaceRef, word for word."""
from __future__ import annotations

from tests._race_ref import RaceRef


class TunedRaceRef(RaceRef):
    def __init__(self, track, plant0, path_weights, tt_weights=None, plan_weights=None, **kw):
        self._b = 0
        self._path_w, self._tt_w, self._plan_w = path_weights, tt_weights, plan_weights
        self._nominal = {}
        super().__init__(track, plant0, **kw)

    def _of(self, name, per_vehicle):
        return self._nominal[name] if per_vehicle is None else per_vehicle[self._b]

    path_tuning = property(lambda self: self._of("path", self._path_w), lambda self, v: self._nominal.__setitem__("path", v))
    tt_tuning = property(lambda self: self._of("tt", self._tt_w), lambda self, v: self._nominal.__setitem__("tt", v))
    plan_weights = property(lambda self: self._of("plan", self._plan_w), lambda self, v: self._nominal.__setitem__("plan", v))

    def _solve_path(self, b, x_meas, seed):
        self._b = b
        return super()._solve_path(b, x_meas, seed)

    def _solve_tt_event(self, b, x_meas):
        self._b = b
        return super()._solve_tt_event(b, x_meas)
