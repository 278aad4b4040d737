"""CPU: the race engine's C ABI (struct layout, exports) and its host replay (tests/_race_ref.py) against
tests/golden/cascade.npz, which was made with the reference's classes: lap 0 up to and including the lap event, then 60
racing ticks of planner + trajectory-tracking controller + plant."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests._golden import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_race_config_layout_and_exports(tmp_path):
    from lpvmpc import _ffi
    src = tmp_path / "race.c"
    src.write_text('#include "lpvmpc.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(){printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(lpvmpc_race_config), offsetof(lpvmpc_race_config, n_sub_lap0),'
                   ' offsetof(lpvmpc_race_config, n_sub), offsetof(lpvmpc_race_config, q9_swap), offsetof(lpvmpc_race_config, half_width),'
                   ' offsetof(lpvmpc_race_config, dt_sim), offsetof(lpvmpc_race_config, mu_sim)); return 0;}\n')
    exe = tmp_path / "race"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    R = _ffi.RaceConfig
    assert got == [C.sizeof(R), R.n_sub_lap0.offset, R.n_sub.offset, R.q9_swap.offset, R.half_width.offset, R.dt_sim.offset, R.mu_sim.offset]
    names = ("lpvmpc_solve_batch_masked", "lpvmpc_race_default_config", "lpvmpc_race_init", "lpvmpc_race_tick", "lpvmpc_race_read",
             "lpvmpc_race_laps")
    lib = _ffi.load()
    for n in names:
        assert n in _ffi.EXPORTS and hasattr(lib, n), n
    c = _ffi.default_race_config()
    assert (c.laps, c.n_sub_lap0, list(c.n_sub), c.q9_swap, c.dt_sim, c.mu_sim) == (1, 7, [7, 7, 6], 1, 0.005, 0.05)
    import lpvmpc
    assert lpvmpc.RaceFleet is not None


def test_race_replay_reproduces_the_cascade_fixture():
    """One vehicle from pre_plant[0] with HalfTrack = 1: the 17 lap-0 ticks (seed ticks, LPV ticks, the event tick) and the 60
    racing ticks, to the bars of the existing cascade tests."""
    import lpvmpc
    from tests._race_ref import RaceRef
    c = load("cascade")
    mp = lpvmpc.Map("L_shape", 0.2)
    ref = RaceRef(mp.PointAndTangent, c["pre_plant"][0][None], half_track0=1, laps=5, half_width=mp.halfWidth, slack=mp.slack)
    P = int(c["pre_ticks"])
    for t in range(P):
        assert np.max(np.abs(ref.plant[0] - c["pre_plant"][t])) <= 2e-6, t
        ref.tick()
        assert np.max(np.abs(ref.local[0] - c["pre_local"][t])) <= 2e-6, t
        assert np.max(np.abs(ref.cmd[0] - c["pre_cmd"][t])) <= 2e-5, t
        assert ref.lap[0] == c["pre_lap"][t], t
    assert ref.event_tick[0] == P - 1 and ref.phase[0] == 1
    assert np.max(np.abs(ref.plant[0] - c["plant0"])) <= 2e-6
    worst = dict(plant=0.0, local=0.0, cmd=0.0)
    for k in range(60):
        worst["plant"] = max(worst["plant"], float(np.max(np.abs(ref.plant[0] - c["ctrl_plant"][k]))))
        ref.tick()
        worst["local"] = max(worst["local"], float(np.max(np.abs(ref.local[0] - c["ctrl_local"][k]))))
        worst["cmd"] = max(worst["cmd"], float(np.max(np.abs(ref.cmd[0] - c["ctrl_cmd"][k]))))
        assert ref.lap[0] == c["ctrl_lap"][k] and ref.status[0] == c["ctrl_status"][k], k
    print("race replay vs cascade.npz racing ticks:", worst)
    assert max(worst.values()) <= 2e-2
