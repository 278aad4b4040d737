"""CPU: the race event log's reference (tests/_events_ref.py) against its own definitions and the heats' reference, the ring's
arithmetic, the header against _ffi, the exported symbols, the Python-side refusals, and what the crafted cases contain."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import _events_cases as K
from tests import _events_ref as R
from tests import _heats_cases as HK
from tests import _heats_ref as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPTS = {
    "crafted": K.crafted,
    "reversal": K.reversal,
    "all_and_none": lambda: K.all_and_none(65),
    "random": lambda: K.random_script(70, K.interleaved_heats(70, 8), 8, 5, heats_on=lambda t: t not in (3, 4), walls_on=lambda t: t != 5),
}


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_the_order_is_strictly_increasing_and_the_counts_add_up(name):
    per_tick, ref = K.run_ref(SCRIPTS[name]())
    flat = [e for evs in per_tick for e in evs]
    keys = [R.key(e) for e in flat]
    assert all(a < b for a, b in zip(keys, keys[1:]))
    assert ref.total == len(flat) and int(ref.count_total.sum()) == len(flat)
    for e in flat:
        assert 1 <= e[1] <= 8 and 0 <= e[2] < ref.B
        if e[1] == R.PASS:
            assert e[3] != e[2] and e[4] < e[5]                                 # the passer is in front afterwards


def test_the_reversal_has_the_counts_the_issue_names():
    per_tick, _ = K.run_ref(K.reversal())
    assert [len(e) for e in per_tick] == [0, 32640, 0]
    assert sum(1 for e in per_tick[1] if e[2] == 255) == 255 and all(e[1] == R.PASS for e in per_tick[1])


@pytest.mark.parametrize("scale", sorted(HK.SEQUENCES))
def test_pass_events_are_the_increments_of_the_heats_own_counters(scale):
    """The heats' reference on its scripted poses; its planes feed the log's reference: per vehicle and tick the PASS events with
    VEHICLE = b are the increment of passes[b], those with OTHER = b the increment of passed[b]; and the sequence has passes."""
    static, ticks = HK.sequence(HK.SEQUENCES[scale])
    B = static["heat"].shape[0]
    heats = HR.HeatsRef(static["heat"], static["L"], static["turns0"])
    log = R.EventsRef(B)
    passes = np.zeros(B, int); passed = np.zeros(B, int)
    seen = 0
    for t, k in enumerate(ticks):
        o = heats.step(t, k["pose"], k["s"], k["inside"], k["phase"])
        f = np.array([o[n] for n in ("progress", "gap_ahead", "gap_leader", "clearance", "min_clearance")], float)
        i = np.array([o[n] for n in ("position", "ahead", "nearest", "contact", "contact_ticks", "first_contact_tick", "passes", "passed",
                                     "turns", "class")], int)
        evs = log.step(t, k["phase"], np.zeros(B, int), np.zeros(B), dict(f64=f, i32=i), static["heat"])
        by = np.zeros(B, int); of = np.zeros(B, int)
        for e in evs:
            if e[1] == R.PASS:
                by[e[2]] += 1; of[e[3]] += 1
        assert np.array_equal(by, o["passes"] - passes) and np.array_equal(of, o["passed"] - passed), t
        passes, passed = o["passes"].copy(), o["passed"].copy()
        seen += int(by.sum())
    assert seen >= 3 and seen == passes.sum()


def test_ring_arithmetic():
    """Capacity 1, capacity 7 with ticks of 0, 3 and 20 events (one larger than the ring), and a capacity that does not divide the
    total: total, kept, oldest-first, and never two writes of a tick in one slot (Ring.push_tick asserts it)."""
    evs = [(t, 1, b, -1, b, 0, 0.0, 0.0) for t, n in enumerate((0, 3, 20, 0, 5)) for b in range(n)]
    by_tick = [[e for e in evs if e[0] == t] for t in range(5)]
    for cap in (1, 7, 5, 28, 100):
        ring = R.Ring(cap)
        flat = []
        for tick in by_tick:
            before = ring.writes
            ring.push_tick(tick)
            assert ring.writes - before == min(len(tick), cap)                  # a tick larger than the ring keeps exactly its last cap
            flat += tick
            assert ring.total == len(flat) and ring.kept == min(len(flat), cap)
            assert ring.read() == flat[len(flat) - ring.kept:]
            assert ring.read(2) == flat[len(flat) - min(2, ring.kept):]
        assert ring.read(0) == []


def test_header_and_ffi_agree(tmp_path):
    from lpvmpc import _ffi
    names = ["I32", "F64", "OUT_I32", "CARRY_F64", "CARRY_I32", "ALL_KINDS", "LAP", "FINISH", "LOST", "PASS", "CONTACT_BEGIN", "CONTACT_END",
             "WALL_HIT", "WALL_CLEAR", "TICK", "KIND", "VEHICLE", "OTHER", "A", "B", "V0", "V1", "COUNT", "COUNT_TOTAL"]
    carry_i = ["FLAGS", "PHASE", "LAP", "POSITION", "CLASS", "CONTACT", "NEAREST", "CONTACT_START", "HIT", "HIT_START", "COUNT_TOTAL"]
    carry_f = ["MIN_CLEARANCE", "MAX_IMPULSE"]
    macros = ["LPVMPC_EVENT_" + n for n in names] + ["LPVMPC_EVENT_CARRY_" + n for n in carry_i + carry_f]
    src = tmp_path / "ev.c"
    src.write_text('#include "lpvmpc.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){\n' +
                   "".join('printf("%%ld\\n", (long)%s);\n' % m for m in macros) +
                   'printf("%zu %zu %zu %zu\\n", sizeof(lpvmpc_event_config), offsetof(lpvmpc_event_config, capacity), '
                   'offsetof(lpvmpc_event_config, kinds), offsetof(lpvmpc_event_config, reserved));\nreturn 0;}\n')
    exe = tmp_path / "ev"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    v = dict(zip(macros, map(int, out[:len(macros)])))
    g = lambda n: v["LPVMPC_EVENT_" + n]
    assert (g("I32"), g("F64"), g("OUT_I32"), g("CARRY_F64"), g("CARRY_I32")) == \
           (_ffi.EVENT_I32, _ffi.EVENT_F64, _ffi.EVENT_OUT_I32, _ffi.EVENT_CARRY_F64, _ffi.EVENT_CARRY_I32) == (6, 2, 2, 2, 11)
    assert g("ALL_KINDS") == _ffi.EVENT_ALL_KINDS == sum(1 << k for k in range(1, 9))
    assert [g(n.upper()) for n in _ffi.EVENT_KIND_NAMES] == list(range(1, 9))
    assert [g(n.upper()) for n in _ffi.EVENT_I32_NAMES] == list(range(6)) and [g(n.upper()) for n in _ffi.EVENT_F64_NAMES] == [0, 1]
    assert [g(n.upper()) for n in _ffi.EVENT_OUT_I32_NAMES] == [0, 1]
    assert [g("CARRY_" + n.upper()) for n in _ffi.EVENT_CARRY_I32_NAMES] == list(range(11)) and len(carry_i) == 11
    assert [g("CARRY_" + n.upper()) for n in _ffi.EVENT_CARRY_F64_NAMES] == [0, 1]
    E = _ffi.EventConfig
    assert [C.sizeof(E), E.capacity.offset, E.kinds.offset, E.reserved.offset] == list(map(int, out[len(macros):])) == [16, 0, 4, 8]
    assert (R.LAP, R.WALL_CLEAR, R.ALL_KINDS) == (g("LAP"), g("WALL_CLEAR"), g("ALL_KINDS"))
    from lpvmpc import events as Ev
    assert Ev.DTYPE.names == _ffi.EVENT_I32_NAMES + _ffi.EVENT_F64_NAMES and Ev.KINDS["wall_clear"] == 8 and Ev.KINDS[4] == "pass"
    assert K.SCAN_WIDTH == int(open(os.path.join(ROOT, "autonomous-racing-lpv-mpp-mpc_amd", "csrc", "events.hpp")).read()
                               .split("constexpr int kEventBlock = ")[1].split(";")[0])


def test_the_library_exports_the_event_log():
    from lpvmpc import _ffi
    lib = _ffi.load()
    for n in ("lpvmpc_event_default_config", "lpvmpc_race_events", "lpvmpc_race_events_read", "lpvmpc_event_step_batch"):
        assert n in _ffi.EXPORTS and hasattr(lib, n), n
    c = _ffi.default_event_config()
    assert (c.capacity, c.kinds, list(c.reserved)) == (65536, _ffi.EVENT_ALL_KINDS, [0, 0])


def test_python_side_refusals_and_views():
    from lpvmpc import _ffi, events as E
    for bad in (0, -1, 2**31, 1.5, True):
        with pytest.raises(ValueError):
            E.event_config(capacity=bad)
    for bad in (1, 0x200, -2, ["overtake"], [0], [9], [True]):
        with pytest.raises(ValueError):
            E.event_config(kinds=bad)
    with pytest.raises(ValueError):
        E.as_config(_ffi.EventConfig(4, E.ALL_KINDS, (0, 1)))
    with pytest.raises(TypeError):
        E.as_config(dict(size=4))
    c = E.as_config(dict(capacity=7, kinds=["pass", 7]))
    assert (c.capacity, c.kinds) == (7, (1 << 4) | (1 << 7)) and E.kinds_mask(0) == 0 and E.as_config(None).capacity == 65536
    k = E.new_carry(5)
    assert k["f64"].shape == (2, 5) and k["i32"].shape == (11, 5) and not k["i32"].any() and not k["f64"].any() and k["total"] == 0
    per_tick, _ = K.run_ref(K.crafted())
    i, f = R.arrays(per_tick[1])
    tab = E.events_table(i, f)
    assert tab.shape[0] == len(per_tick[1]) and tab["kind"].tolist() == [e[1] for e in per_tick[1]]
    assert E.filter(tab, kind="pass")["other"].tolist() == [0, 1, 3] and E.filter(tab, kind=("lost", 7), vehicle=[4, 5])["vehicle"].tolist() == [4, 5]
    with pytest.raises(ValueError):
        E.events_table(i, f[:-1])


def test_what_the_crafted_cases_contain():
    per_tick, ref = K.run_ref(K.crafted())
    flat = [e for evs in per_tick for e in evs]
    assert {e[1] for e in flat} == set(range(1, 9))                             # every kind
    assert per_tick[0] == [] and per_tick[-1] == [] and per_tick[2] == [] and per_tick[3] == []    # first sight; holds; a quiet tick
    two = [e[1] for e in per_tick[1] if e[2] == 2]
    assert two == [R.LAP, R.FINISH, R.PASS, R.PASS, R.PASS, R.CONTACT_BEGIN, R.WALL_HIT]         # every kind that can share a tick
    nan = float("nan")
    ends = {(e[1], e[2]): e for e in per_tick[4]}
    assert ends[(R.CONTACT_END, 0)][3:7] == (1, 3, -1, -0.04) and ends[(R.CONTACT_END, 2)][3:7] == (0, 3, -1, -0.03)
    assert ends[(R.WALL_CLEAR, 2)][3:7] == (-1, 3, -1, 0.5) and ends[(R.WALL_CLEAR, 4)][3:7] == (-1, 3, -1, 1.25)
    assert per_tick[1][0][:3] == (1, R.CONTACT_BEGIN, 0)                        # vehicle 0 comes first
    lap = [e for e in per_tick[1] if e[1] == R.LAP][0]
    assert lap[:7] == (1, R.LAP, 2, -1, 1, 2, 231.0) and lap[7] != lap[7]
    hit = [e for e in per_tick[1] if e[1] == R.WALL_HIT and e[2] == 4][0]
    assert hit[3:] == (-1, -1, 3, 0.03, 0.75)
    p = [e for e in per_tick[1] if e[1] == R.PASS][0]
    assert p[2:7] == (2, 0, 0, 1, 0.25)
    # a kinds mask neither writes nor counts, and carries the state: the ends still know their spells
    only, r2 = K.run_ref(K.crafted(), kinds=(1 << R.CONTACT_END) | (1 << R.WALL_CLEAR))
    assert [e for evs in only for e in evs] == [e for e in flat if e[1] in (R.CONTACT_END, R.WALL_CLEAR)] and r2.total == 4
    assert K.run_ref(K.crafted(), kinds=0)[1].total == 0
