"""Per-lap tracking statistics of a race trace, in numpy: the restatement of the race recorder's statistics (csrc/record.hip,
include/lpvmpc.h "Race recorder").  ``lap_stats`` replays a trace in tick order with the recorder's operations -- s = s + x * x,
each product and sum rounded, and max only when |x| exceeds it -- so on a stride-1 trace of a recorded race it reproduces
``BatchedSolver.race_lap_stats`` word for word.  It applies as well to host replays laid out as a trace (dict of [n, B] arrays named
as ``_ffi.REC_F64_NAMES`` / ``REC_I32_NAMES`` plus ``tick`` [n]); on a trace with gaps only the ticks in it count.
``standings_table`` turns the standings of a race's heats (``BatchedSolver.race_standings``) into the table a user prints."""
from __future__ import annotations

import numpy as np

from . import _ffi

SOLVED = 1          # LPVMPC_SOLVED


def lap_stats(trace, laps, phase0=None, q9_swap=True):
    """Statistics per vehicle and lap 0 .. laps of the ticks in ``trace`` (see include/lpvmpc.h for the definitions).
    ``phase0`` [B]: the vehicles' phases before the first tick of the trace (default 0: nothing had ended), which decides
    whether a vehicle ends within the trace (end_tick) or before it (-1), and whether its first tick is its lap event.
    ``q9_swap``: the race's (default on, as the race's): the lap-0 branch then stores ey in local slot 3 and epsi in slot 5, and
    ey / epsi are taken from there on the ticks it measured (phase 0 after the tick, or the event tick: phase 0 -> 1).
    Returns the dict of ``BatchedSolver.race_lap_stats``."""
    src = np.asarray(trace["src"])
    n, B = src.shape
    L1 = int(laps) + 1
    f = np.zeros((B, L1, _ffi.LAPSTAT_F64))
    i = np.zeros((B, L1, _ffi.LAPSTAT_I32), np.int32)
    end = np.full(B, -1, np.int32)
    prev = np.zeros(B, np.int64) if phase0 is None else np.asarray(phase0, np.int64).copy()
    rows = np.arange(B)
    for t in range(n):
        ph = np.asarray(trace["phase"][t], np.int64)
        swapped = bool(q9_swap) & ((ph == 0) | ((ph == 1) & (prev == 0)))        # ticks measured by the lap-0 branch
        ended = (prev < 2) & (ph >= 2)
        end[ended] = int(trace["tick"][t])
        prev = ph
        lap = np.asarray(trace["lap"][t], np.int64)
        c = (src[t] >= 0) & (lap >= 0) & (lap <= laps)
        b, l = rows[c], lap[c]
        vx = trace["local_vx"][t][c]
        ev = vx - trace["vel_ref"][t][c]
        sw = swapped[c]
        ey = np.where(sw, trace["local_epsi"][t][c], trace["local_ey"][t][c])
        epsi = np.where(sw, trace["local_ey"][t][c], trace["local_epsi"][t][c])
        tey = trace["track_ey"][t][c]
        F = f[b, l]
        F[:, _ffi.LAPSTAT_SSE_V] = F[:, _ffi.LAPSTAT_SSE_V] + ev * ev
        F[:, _ffi.LAPSTAT_SSE_EY] = F[:, _ffi.LAPSTAT_SSE_EY] + ey * ey
        F[:, _ffi.LAPSTAT_SSE_EPSI] = F[:, _ffi.LAPSTAT_SSE_EPSI] + epsi * epsi
        a = np.abs(ey)
        F[:, _ffi.LAPSTAT_MAX_EY] = np.where(a > F[:, _ffi.LAPSTAT_MAX_EY], a, F[:, _ffi.LAPSTAT_MAX_EY])
        F[:, _ffi.LAPSTAT_SUM_VX] = F[:, _ffi.LAPSTAT_SUM_VX] + vx
        a = np.abs(tey)
        F[:, _ffi.LAPSTAT_MAX_EY_TRACK] = np.where(a > F[:, _ffi.LAPSTAT_MAX_EY_TRACK], a, F[:, _ffi.LAPSTAT_MAX_EY_TRACK])
        f[b, l] = F
        it, st = np.asarray(trace["iters"][t])[c], np.asarray(trace["status"][t])[c]
        pl = np.asarray(trace["plan_iters"][t])[c] >= 0
        pit, pst = np.asarray(trace["plan_iters"][t])[c], np.asarray(trace["plan_status"][t])[c]
        I = i[b, l]
        I[:, _ffi.LAPSTAT_TICKS] += 1
        I[:, _ffi.LAPSTAT_CTRL_ITERS] += it
        I[:, _ffi.LAPSTAT_CTRL_ITERS_MAX] = np.maximum(I[:, _ffi.LAPSTAT_CTRL_ITERS_MAX], it)
        I[:, _ffi.LAPSTAT_CTRL_NOT_SOLVED] += st != SOLVED
        I[:, _ffi.LAPSTAT_PLAN_TICKS] += pl
        I[:, _ffi.LAPSTAT_PLAN_ITERS] += np.where(pl, pit, 0)
        I[:, _ffi.LAPSTAT_PLAN_ITERS_MAX] = np.where(pl, np.maximum(I[:, _ffi.LAPSTAT_PLAN_ITERS_MAX], pit), I[:, _ffi.LAPSTAT_PLAN_ITERS_MAX])
        I[:, _ffi.LAPSTAT_PLAN_NOT_SOLVED] += pl & (pst != SOLVED)
        I[:, _ffi.LAPSTAT_OFF_TRACK] += np.asarray(trace["inside"][t])[c] == 0
        i[b, l] = I
    return _ffi.lap_stats_dict(f, i, end)


def standings_table(standings, heat):
    """Per heat, the vehicles in finishing / running order with their gaps: ``standings`` a ``BatchedSolver.race_standings`` /
    ``heat_step`` dict, ``heat`` [B] the heats as they were attached (-1: none).  Returns {heat index: dict(vehicle, position, cls,
    progress, gap_ahead, gap_leader, passes, passed, contact_ticks, min_clearance)} with every array in position order.  Host only.
    Raises ValueError when the positions of a heat are not 0 .. n-1 (standings of another attachment, or read before the first tick)."""
    from .heats import check_heats
    pos = np.asarray(standings["position"])
    h = check_heats(heat, pos.shape[0])
    out = {}
    for g in np.unique(h[h >= 0]):
        veh = np.nonzero(h == g)[0]
        p = pos[veh]
        if not np.array_equal(np.sort(p), np.arange(veh.shape[0])):
            raise ValueError("standings_table: the positions of heat %d are not a permutation of 0 .. %d" % (int(g), veh.shape[0] - 1))
        v = veh[np.argsort(p)]
        row = dict(vehicle=v, position=pos[v], cls=np.asarray(standings["class"])[v])
        for k in ("progress", "gap_ahead", "gap_leader", "passes", "passed", "contact_ticks", "min_clearance"):
            row[k] = np.asarray(standings[k])[v]
        out[int(g)] = row
    return out


def add_rmse(stats):
    """stats (a ``lap_stats`` / ``race_lap_stats`` dict) with rmse_v, rmse_ey, rmse_epsi [B, laps+1] (RMSE_ve, RMSE_ye,
    RMSE_thetae of controllerMain.py) and mean_vx; NaN where a lap has no counted tick."""
    n = stats["ticks"].astype(float)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.where(n > 0, n, np.nan)
        out = dict(stats)
        out["rmse_v"] = np.sqrt(stats["sse_v"] / d)
        out["rmse_ey"] = np.sqrt(stats["sse_ey"] / d)
        out["rmse_epsi"] = np.sqrt(stats["sse_epsi"] / d)
        out["mean_vx"] = stats["sum_vx"] / d
    return out
