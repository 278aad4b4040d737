"""Interactions (include/lpvmpc.h, "Interactions"): host-side helpers of ``BatchedSolver.race_interactions`` /
``race_interactions_read`` / ``interaction_step`` -- the configuration with the checks that need no device, the carried state of the
batch form, the named views of the output planes, and ``grid``, which puts a heat on the track without two footprints at one pose."""
from __future__ import annotations

import math

import numpy as np

from . import _ffi
from ._planes import blank_carry, planes_dict

# lpvmpc_interaction_default_config: invented values of the right order for a 1:10 car, nothing in the reference fixes them
DEFAULTS = dict(draft_gain=0.3, wake_length=3.0, wake_half_width=0.3, contact=1, restitution=0.2, push=0.5)


def interaction_config(**words):
    """An ``_ffi.InteractionConfig`` from the defaults and ``words`` (draft_gain, wake_length, wake_half_width, contact, restitution,
    push).  Raises ValueError for what lpvmpc_race_interactions refuses: an unknown word, a word that is not finite, draft_gain /
    restitution / push outside [0, 1], wake_length / wake_half_width not > 0, contact other than 0 / 1."""
    unknown = sorted(set(words) - set(DEFAULTS))
    if unknown:
        raise ValueError("interaction_config: unknown word(s) %s (have %s)" % (unknown, sorted(DEFAULTS)))
    w = dict(DEFAULTS)
    w.update(words)
    c = w["contact"]
    if isinstance(c, (bool, np.bool_)):
        c = int(c)
    if not isinstance(c, (int, np.integer)) or c not in (0, 1):
        raise ValueError("interaction_config: contact = %r must be 0 or 1" % (w["contact"],))
    for k in ("draft_gain", "wake_length", "wake_half_width", "restitution", "push"):
        w[k] = float(w[k])
        if not math.isfinite(w[k]):
            raise ValueError("interaction_config: %s = %g is not finite" % (k, w[k]))
    for k in ("draft_gain", "restitution", "push"):
        if not 0.0 <= w[k] <= 1.0:
            raise ValueError("interaction_config: %s = %g must lie in [0, 1]" % (k, w[k]))
    for k in ("wake_length", "wake_half_width"):
        if not w[k] > 0.0:
            raise ValueError("interaction_config: %s = %g must be > 0" % (k, w[k]))
    return _ffi.InteractionConfig(w["draft_gain"], w["wake_length"], w["wake_half_width"], int(c), 0, w["restitution"], w["push"])


def as_config(cfg):
    """None (the defaults), a dict of words or an ``_ffi.InteractionConfig`` -> a checked ``_ffi.InteractionConfig``."""
    if cfg is None:
        return interaction_config()
    if isinstance(cfg, dict):
        return interaction_config(**cfg)
    return interaction_config(**{k: getattr(cfg, k) for k in DEFAULTS})


def new_carry(B):
    """The carried state "just attached" of ``BatchedSolver.interaction_step`` for B vehicles: no impulse, no hit (first_hit_tick -1),
    no drafting tick."""
    return blank_carry(B, _ffi.INTER_CARRY_F64, _ffi.INTER_CARRY_I32_NAMES, ("first_hit_tick",))


def interactions_dict(f, i):
    """Output planes f [INTER_F64, B], i [INTER_I32, B] -> dict of [B] arrays named as _ffi.INTER_F64_NAMES / INTER_I32_NAMES and the
    planes themselves (f64, i32)."""
    return planes_dict(f, i, _ffi.INTER_F64_NAMES, _ffi.INTER_I32_NAMES)


def grid(track, n, gap, stagger=0.0, vx=1.0, position=None):
    """A starting grid of n cars on ``track`` (a ``track.Map``): car k stands ``(k + 1) * gap`` metres behind the line s = 0 along the
    centre line, cars alternating +stagger / -stagger in ey (car 0 at +stagger), each heading along the track at speed ``vx``.  Returns
    (plant0 [n, 8], turns0 [n]): the plant rows of ``RaceFleet`` / ``race_init``, and -1 for every car, since all stand behind the line
    (``race_heats(turns0=)``).  The poses come from the package's global-position transform, ``track.getGlobalPosition`` (a device
    kernel); ``position``: another callable (s, ey) -> (x, y, theta)."""
    n = int(n)
    gap, stagger = float(gap), float(stagger)
    L = float(track.TrackLength)
    if n < 1 or not (math.isfinite(gap) and gap > 0) or not math.isfinite(stagger):
        raise ValueError("grid: n = %d must be >= 1, gap = %g finite and > 0, stagger = %g finite" % (n, gap, stagger))
    if n * gap >= L:
        raise ValueError("grid: %d cars %g m apart do not fit on a lap of %g m" % (n, gap, L))
    if abs(stagger) > float(track.halfWidth):
        raise ValueError("grid: stagger = %g is wider than the track's half width %g" % (stagger, float(track.halfWidth)))
    where = track.getGlobalPosition if position is None else position
    plant0 = np.zeros((n, 8))
    for k in range(n):
        x, y, th = where(L - (k + 1) * gap, stagger if k % 2 == 0 else -stagger)
        plant0[k] = [x, y, float(vx), 0.0, 0.0, 0.0, th, 0.0]
    return plant0, np.full(n, -1, np.int32)
