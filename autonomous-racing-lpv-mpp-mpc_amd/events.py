"""Race event log (include/lpvmpc.h, "Race event log"): host-side helpers of ``BatchedSolver.race_events`` / ``race_events_read`` /
``event_step`` -- the kinds, the configuration with the checks that need no device, the carried state of the batch form, and the
events as a structured numpy array with named fields."""
from __future__ import annotations

import numpy as np

from . import _ffi
from ._planes import blank_carry

# name <-> number of an event's kind (LPVMPC_EVENT_LAP ... LPVMPC_EVENT_WALL_CLEAR)
KINDS = {name: k + 1 for k, name in enumerate(_ffi.EVENT_KIND_NAMES)}
KINDS.update({k: name for name, k in list(KINDS.items())})
ALL_KINDS = _ffi.EVENT_ALL_KINDS
DEFAULT_CAPACITY = 65536                 # lpvmpc_event_default_config
I32_NAMES, F64_NAMES = _ffi.EVENT_I32_NAMES, _ffi.EVENT_F64_NAMES
CARRY_F64_NAMES, CARRY_I32_NAMES = _ffi.EVENT_CARRY_F64_NAMES, _ffi.EVENT_CARRY_I32_NAMES
# an event as a record: the six integer words, then the two doubles
DTYPE = np.dtype([(k, np.int32) for k in I32_NAMES] + [(k, np.float64) for k in F64_NAMES])


def kinds_mask(kinds):
    """The kinds word: None (every kind), an integer mask (bit k selects kind k), or an iterable of kind names / numbers.  Raises
    ValueError for a bit outside 1 .. 8 or an unknown name, as lpvmpc_race_events refuses them."""
    if kinds is None:
        return ALL_KINDS
    if isinstance(kinds, (int, np.integer)) and not isinstance(kinds, (bool, np.bool_)):
        m = int(kinds)
    else:
        m = 0
        for k in kinds:
            if isinstance(k, str):
                if k not in KINDS:
                    raise ValueError("event_config: unknown kind %r (have %s)" % (k, list(_ffi.EVENT_KIND_NAMES)))
                k = KINDS[k]
            if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 8:
                raise ValueError("event_config: kind %r is not a kind's name or a number in 1 .. 8" % (k,))
            m |= 1 << int(k)
    if m < 0 or m & ~ALL_KINDS:
        raise ValueError("event_config: kinds = 0x%x has a bit outside 1 .. 8" % m)
    return m


def event_config(capacity=DEFAULT_CAPACITY, kinds=None):
    """An ``_ffi.EventConfig``: the ring keeps the last ``capacity`` events of the ``kinds`` selected (``kinds_mask``).  Raises
    ValueError for what lpvmpc_race_events refuses: capacity < 1 or beyond int32, a kinds bit outside 1 .. 8."""
    if isinstance(capacity, (bool, np.bool_)) or not isinstance(capacity, (int, np.integer)) or not 1 <= int(capacity) <= 2**31 - 1:
        raise ValueError("event_config: capacity = %r must be an integer in [1, 2^31)" % (capacity,))
    return _ffi.EventConfig(int(capacity), kinds_mask(kinds), (0, 0))


def as_config(cfg):
    """None (the defaults), a dict of ``event_config``'s arguments or an ``_ffi.EventConfig`` -> a checked ``_ffi.EventConfig``."""
    if cfg is None:
        return event_config()
    if isinstance(cfg, dict):
        return event_config(**cfg)
    if any(int(r) != 0 for r in cfg.reserved):
        raise ValueError("event_config: reserved = %r must be 0" % (list(cfg.reserved),))
    return event_config(cfg.capacity, cfg.kinds)


def new_carry(B):
    """The carried state "just attached" of ``BatchedSolver.event_step`` for B vehicles: all zero, and ``total`` 0."""
    c = blank_carry(B, _ffi.EVENT_CARRY_F64, CARRY_I32_NAMES)
    c["total"] = 0
    return c


def events_table(i32, f64):
    """Events i32 [m, 6] / f64 [m, 2] -> a structured array [m] with the fields tick, kind, vehicle, other, a, b, v0, v1."""
    i = np.asarray(i32, np.int32).reshape(-1, _ffi.EVENT_I32)
    f = np.asarray(f64, np.float64).reshape(-1, _ffi.EVENT_F64)
    if i.shape[0] != f.shape[0]:
        raise ValueError("events_table: %d integer rows, %d double rows" % (i.shape[0], f.shape[0]))
    t = np.empty(i.shape[0], DTYPE)
    for c, k in enumerate(I32_NAMES):
        t[k] = i[:, c]
    for c, k in enumerate(F64_NAMES):
        t[k] = f[:, c]
    return t


def filter(table, kind=None, vehicle=None):
    """The rows of an ``events_table`` of the given kind(s) (names or numbers) and vehicle(s), in the table's order."""
    keep = np.ones(table.shape[0], bool)
    if kind is not None:
        ks = [kind] if isinstance(kind, (str, int, np.integer)) else list(kind)
        ks = [KINDS[k] if isinstance(k, str) else int(k) for k in ks]
        keep &= np.isin(table["kind"], ks)
    if vehicle is not None:
        keep &= np.isin(table["vehicle"], np.atleast_1d(np.asarray(vehicle)))
    return table[keep]
