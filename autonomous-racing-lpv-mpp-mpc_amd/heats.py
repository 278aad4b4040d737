"""Heats (include/lpvmpc.h, "Heats"): host-side helpers of ``BatchedSolver.race_heats`` / ``race_standings`` / ``heat_step`` -- the
checks that need no device, the carried state of the batch form, and the named views of the standings planes."""
from __future__ import annotations

import numpy as np

from . import _ffi
from ._planes import blank_carry, planes_dict


def check_heats(heat, B, track_of=None):
    """heat [B] as a contiguous int32 array: the heat of each vehicle, -1 for none.  Raises ValueError for what lpvmpc_race_heats
    refuses: another length than B, an index below -1, a heat of more than 256 members and, with ``track_of`` [B], a heat whose
    members are on different tracks."""
    h = np.asarray(heat)
    if h.ndim != 1 or h.shape[0] != int(B):
        raise ValueError("heat must have one entry per vehicle (%d), got shape %s" % (B, h.shape))
    if h.dtype.kind not in "iu":
        if h.dtype.kind != "f" or np.any(h != np.round(h)):
            raise ValueError("heat must hold integers")
    h = np.ascontiguousarray(h, np.int32)
    if np.any(h < -1):
        raise ValueError("heat index %d (-1: no heat)" % int(h.min()))
    ids, counts = np.unique(h[h >= 0], return_counts=True)
    if counts.size and counts.max() > _ffi.HEAT_MAX:
        raise ValueError("heat %d has %d members, at most %d" % (int(ids[np.argmax(counts)]), int(counts.max()), _ffi.HEAT_MAX))
    if track_of is not None:
        of = np.asarray(track_of).reshape(-1)
        for g in ids:
            on = np.unique(of[h == g])
            if on.size > 1:
                raise ValueError("heat %d spans tracks %s: a heat shares one track" % (int(g), on.tolist()))
    return h


def check_extents(half_length, half_width):
    hl, hw = float(half_length), float(half_width)
    if not (np.isfinite(hl) and hl > 0 and np.isfinite(hw) and hw > 0):
        raise ValueError("half_length = %g, half_width = %g must be finite and > 0" % (hl, hw))
    return hl, hw


def new_carry(B, turns0=None, phase0=None, lines=0):
    """The carried state "just attached" of ``BatchedSolver.heat_step`` for B vehicles: flag word 0, TURNS = ``turns0`` (default 0),
    PHASE = ``phase0`` (the phases before the attach, default 0: running).  ``lines`` > 0 adds the line tables line_tick / line_pos
    [B, lines] (-1), which heat_step fills from the carried crossing count as the race's kernel does on the device."""
    c = blank_carry(B, _ffi.HEAT_CARRY_F64, _ffi.HEAT_CARRY_I32_NAMES)
    if turns0 is not None:
        c["i32"][_ffi.HEAT_CARRY_I32_NAMES.index("turns")] = np.asarray(turns0, np.int32).reshape(B)
    if phase0 is not None:
        c["i32"][_ffi.HEAT_CARRY_I32_NAMES.index("phase")] = np.asarray(phase0, np.int32).reshape(B)
    if lines:
        c["line_tick"] = np.full((B, int(lines)), -1, np.int32)
        c["line_pos"] = np.full((B, int(lines)), -1, np.int32)
    return c


def standings_dict(f, i, line_tick=None, line_pos=None):
    """Standings planes f [HEAT_F64, B], i [HEAT_I32, B] -> dict of [B] arrays named as _ffi.HEAT_F64_NAMES / HEAT_I32_NAMES, the
    planes themselves (f64, i32) and the line tables."""
    out = planes_dict(f, i, _ffi.HEAT_F64_NAMES, _ffi.HEAT_I32_NAMES)
    if line_tick is not None:
        out.update(line_tick=line_tick, line_pos=line_pos)
    return out
