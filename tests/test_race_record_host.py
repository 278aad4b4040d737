"""CPU: the race recorder's host side -- the ctypes mirror of lpvmpc_race_record_config, the channel constants against
include/lpvmpc.h, and telemetry.lap_stats (the numpy restatement of the recorder's per-lap statistics) on a hand-computed trace
and on a trace assembled from the host replay of the race (tests/_race_ref.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lpvmpc.h")


def header_defines(prefix):
    text = open(HEADER).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(%s\w+)\s+(-?\d+)" % prefix, text)}


def test_config_struct_layout(tmp_path):
    from lpvmpc import _ffi
    src = tmp_path / "rec.c"
    src.write_text('#include "lpvmpc.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(){printf("%zu %zu %zu\\n", sizeof(lpvmpc_race_record_config), offsetof(lpvmpc_race_record_config, capacity),'
                   ' offsetof(lpvmpc_race_record_config, stride)); return 0;}\n')
    exe = tmp_path / "rec"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, oc, os_ = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    R = _ffi.RaceRecordConfig
    assert (C.sizeof(R), R.capacity.offset, R.stride.offset) == (size, oc, os_)


def test_channel_constants_match_the_header():
    from lpvmpc import _ffi
    d = header_defines("LPVMPC_REC_")
    d.update(header_defines("LPVMPC_LAPSTAT_"))
    assert len(d) == (2 + 6 + 8) + (2 + 6 + 9)
    for name, v in d.items():
        assert getattr(_ffi, name[len("LPVMPC_"):]) == v, name
    assert len(_ffi.REC_F64_NAMES) == _ffi.REC_F64 and len(_ffi.REC_I32_NAMES) == _ffi.REC_I32
    assert len(_ffi.LAPSTAT_F64_NAMES) == _ffi.LAPSTAT_F64 and len(_ffi.LAPSTAT_I32_NAMES) == _ffi.LAPSTAT_I32
    # the named channels sit where the group constants say
    n = _ffi.REC_F64_NAMES
    assert n[_ffi.REC_PLANT] == "x" and n[_ffi.REC_LOCAL] == "local_vx" and n[_ffi.REC_CMD] == "servo"
    assert n[_ffi.REC_REF] == "x_ref" and n[_ffi.REC_TRACK] == "track_s" and n[_ffi.REC_EST] == "est_vx"
    for k in ("phase", "lap", "src", "iters", "status", "plan_iters", "plan_status", "inside"):
        assert _ffi.REC_I32_NAMES.index(k) == getattr(_ffi, "REC_" + k.upper())
    for k in _ffi.LAPSTAT_F64_NAMES:
        assert _ffi.LAPSTAT_F64_NAMES.index(k) == getattr(_ffi, "LAPSTAT_" + k.upper())
    for k in _ffi.LAPSTAT_I32_NAMES:
        assert _ffi.LAPSTAT_I32_NAMES.index(k) == getattr(_ffi, "LAPSTAT_" + k.upper())


def synthetic_trace():
    """Three vehicles, laps = 1, ticks 0 1 2 3 5 6 (a gap at 4).  Vehicle 0: lap 0 on ticks 0-1, its lap event on tick 2 (counted
    in lap 1), one racing tick with a planner solve, finishing on tick 5 (not counted), frozen on tick 6.  Vehicle 1: lap 0, lost on
    tick 3.  Vehicle 2: finished before the trace."""
    tick = np.array([0, 1, 2, 3, 5, 6])
    cols = dict(  # per tick: vehicle 0, 1, 2
        phase=[[0, 0, 2], [0, 0, 2], [1, 0, 2], [1, 3, 2], [2, 3, 2], [2, 3, 2]],
        lap=[[0, 0, 2], [0, 0, 2], [1, 0, 2], [1, 0, 2], [2, 0, 2], [2, 0, 2]],
        src=[[0, 0, -1], [0, 0, -1], [1, 0, -1], [1, -1, -1], [-1, -1, -1], [-1, -1, -1]],
        iters=[[10, 3, 0], [20, 4, 0], [5, 5, 0], [7, 0, 0], [0, 0, 0], [0, 0, 0]],
        status=[[1, 1, 1], [2, 1, 1], [1, 4, 1], [1, 4, 1], [1, 4, 1], [1, 4, 1]],
        plan_iters=[[-1, -1, -1], [-1, -1, -1], [-1, -1, -1], [30, -1, -1], [40, -1, -1], [-1, -1, -1]],
        plan_status=[[-1, -1, -1], [-1, -1, -1], [-1, -1, -1], [1, -1, -1], [3, -1, -1], [-1, -1, -1]],
        inside=[[1, 1, 1], [1, 1, 1], [0, 1, 1], [1, 0, 1], [1, 0, 1], [1, 0, 1]],
        local_vx=[[1, 1, 5], [2, 1, 5], [1.5, 1, 5], [3, 1, 5], [9, 1, 5], [9, 1, 5]],
        vel_ref=[[1, 1, 1], [1, 1, 1], [1, 1, 1], [2, 1, 1], [2, 1, 1], [2, 1, 1]],
        local_ey=[[0.5, 1, 3], [-1, 2, 3], [0.25, 0, 3], [0.5, 0, 3], [7, 0, 3], [7, 0, 3]],
        local_epsi=[[0.25, 0, 1], [0, 0, 1], [0.5, 0, 1], [-0.5, 0, 1], [7, 0, 1], [7, 0, 1]],
        track_ey=[[0.1, 0.5, 2], [-0.3, 0.5, 2], [10000, 0.5, 2], [0.2, 10000, 2], [9, 10000, 2], [9, 10000, 2]],
    )
    tr = {k: np.array(v, np.float64 if k in ("local_vx", "vel_ref", "local_ey", "local_epsi", "track_ey") else np.int32)
          for k, v in cols.items()}
    tr["tick"] = tick
    return tr


def test_lap_stats_by_hand():
    from lpvmpc import telemetry
    s = telemetry.lap_stats(synthetic_trace(), 1, phase0=[0, 0, 2], q9_swap=False)
    assert s["f64"].shape == (3, 2, 6) and s["i32"].shape == (3, 2, 9) and s["i32"].dtype == np.int32
    np.testing.assert_array_equal(s["end_tick"], [5, 3, -1])
    # vehicle 0, lap 0: ticks 0, 1
    assert s["f64"][0, 0].tolist() == [1.0, 1.25, 0.0625, 1.0, 3.0, 0.3]
    assert s["i32"][0, 0].tolist() == [2, 30, 20, 1, 0, 0, 0, 0, 0]
    # vehicle 0, lap 1: the event tick and one racing tick with a planner solve (the finishing tick and its planner solve do not count)
    assert s["f64"][0, 1].tolist() == [1.25, 0.3125, 0.5, 0.5, 4.5, 10000.0]
    assert s["i32"][0, 1].tolist() == [2, 12, 7, 0, 1, 30, 30, 0, 1]
    # vehicle 1: three lap-0 ticks, then lost
    assert s["f64"][1, 0].tolist() == [0.0, 5.0, 0.0, 2.0, 3.0, 0.5]
    assert s["i32"][1, 0].tolist() == [3, 12, 5, 1, 0, 0, 0, 0, 0]
    assert not s["f64"][1, 1].any() and not s["i32"][1, 1].any()
    # vehicle 2: ended before the trace
    assert not s["f64"][2].any() and not s["i32"][2].any()
    # by default nothing had ended before the trace: vehicle 2 then ends on the trace's first tick
    assert telemetry.lap_stats(synthetic_trace(), 1, q9_swap=False)["end_tick"].tolist() == [5, 3, 0]
    r = telemetry.add_rmse(s)
    assert r["rmse_ey"][0, 0] == np.sqrt(1.25 / 2) and r["mean_vx"][0, 1] == 2.25
    assert np.isnan(r["rmse_v"][1, 1]) and np.isnan(r["rmse_epsi"][2, 0])
    # the named [B, laps + 1] views
    assert s["ticks"].tolist() == [[2, 2], [3, 0], [0, 0]] and s["max_ey_track"][0, 1] == 10000.0


def test_lap_stats_swap_the_lap0_branch_slots_with_q9():
    """With q9_swap (the race's default) the lap-0 branch stores ey in local slot 3 and epsi in slot 5 (CMAIN:188): on the ticks it
    measured -- phase 0, and the event tick (phase 0 -> 1), which counts in lap 1 -- ey / epsi are read from there."""
    from lpvmpc import telemetry
    s = telemetry.lap_stats(synthetic_trace(), 1, phase0=[0, 0, 2])
    # vehicle 0, lap 0: ey = slot 3 = (0.25, 0), epsi = slot 5 = (0.5, -1)
    assert s["f64"][0, 0].tolist() == [1.0, 0.0625, 1.25, 0.25, 3.0, 0.3]
    # vehicle 0, lap 1: the event tick swapped (ey 0.5, epsi 0.25), the racing tick not (ey 0.5, epsi -0.5)
    assert s["f64"][0, 1].tolist() == [1.25, 0.5, 0.3125, 0.5, 4.5, 10000.0]
    # vehicle 1, lap 0: ey = slot 3 = 0, epsi = slot 5 = (1, 2, 0)
    assert s["f64"][1, 0].tolist() == [0.0, 0.0, 5.0, 0.0, 3.0, 0.5]
    plain = telemetry.lap_stats(synthetic_trace(), 1, phase0=[0, 0, 2], q9_swap=False)
    assert np.array_equal(s["i32"], plain["i32"]) and np.array_equal(s["end_tick"], plain["end_tick"])
    # a trace that starts on vehicle 0's event tick: the phase before it (0) makes that tick a lap-0-branch tick
    tr = {k: (v[2:] if k != "tick" else v[2:]) for k, v in synthetic_trace().items()}
    assert telemetry.lap_stats(tr, 1, phase0=[0, 0, 2])["f64"][0, 1].tolist() == s["f64"][0, 1].tolist()
    assert telemetry.lap_stats(tr, 1, phase0=[1, 0, 2])["f64"][0, 1].tolist() == plain["f64"][0, 1].tolist()


def test_lap_stats_on_a_host_replay_trace():
    """A trace laid out from the host replay of three vehicles that cross the line within the window."""
    from lpvmpc import Map, telemetry
    from oracle import plant_ref as PR
    from tests._race_observer_ref import start_line_fleet
    from tests._race_ref import RaceRef
    mp = Map("L_shape", 0.2)
    B, T = 3, 40
    plant0 = start_line_fleet(mp.PointAndTangent, B, 7, 0.95, 0.98)
    ref = RaceRef(mp.PointAndTangent, plant0, half_track0=1, laps=1, half_width=mp.halfWidth, slack=mp.slack)
    rows = {k: [] for k in ("phase", "lap", "src", "iters", "status", "plan_iters", "plan_status", "inside", "local_vx", "vel_ref",
                            "local_ey", "local_epsi", "track_ey")}
    for t in range(T):
        before = ref.phase.copy()
        ref.tick()
        solved = (before <= 1) & (ref.phase <= 1)
        vel = np.ones(B)
        for b in range(B):
            if before[b] == 1 and ref.phase[b] == 1:
                vel[b] = ref.casc[b].glue[0].win[3, 0]
        tey, ins = np.zeros(B), np.zeros(B, np.int32)
        for b in range(B):
            p = ref.plant[b]
            _s, tey[b], _e, ins[b] = PR.get_local_position(mp.PointAndTangent, mp.halfWidth, mp.slack, p[0], p[1], p[6])
        for k, v in (("phase", ref.phase), ("lap", ref.lap), ("src", np.where(solved, np.where(ref.lap == 0, 0, 1), -1)),
                     ("iters", ref.iters), ("status", ref.status), ("plan_iters", np.full(B, -1)), ("plan_status", np.full(B, -1)),
                     ("inside", ins), ("local_vx", ref.local[:, 0]), ("vel_ref", vel), ("local_ey", ref.local[:, 5]),
                     ("local_epsi", ref.local[:, 3]), ("track_ey", tey)):
            rows[k].append(np.array(v))
    tr = {k: np.array(v) for k, v in rows.items()}
    tr["tick"] = np.arange(T)
    s = telemetry.lap_stats(tr, 1)
    assert np.all(ref.event_tick >= 0)
    solved = tr["src"] >= 0
    np.testing.assert_array_equal(s["ticks"].sum(axis=1), solved.sum(axis=0))
    for b in range(B):
        e = int(ref.event_tick[b])
        assert s["ticks"][b, 0] == e and s["ticks"][b, 1] == solved[:, b].sum() - e
        acc = 0.0                            # the replay's lap-0 measurement carries quirk Q9: ey in slot 3
        for t in range(e):
            acc = acc + tr["local_epsi"][t, b] * tr["local_epsi"][t, b]
        assert s["sse_ey"][b, 0] == acc
    assert np.all(np.isfinite(telemetry.add_rmse(s)["rmse_v"]))
