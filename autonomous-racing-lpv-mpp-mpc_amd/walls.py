"""Walls (include/lpvmpc.h, "Walls"): host-side helpers of ``BatchedSolver.race_walls`` / ``race_walls_read`` / ``wall_step`` -- the
configuration with the checks that need no device, the carried state of the batch form, the named views of the output planes, and
``corners``, the footprint corners in the header's order."""
from __future__ import annotations

import math

import numpy as np

from . import _ffi
from ._planes import blank_carry, planes_dict

# lpvmpc_wall_default_config: invented values of the right order for a 1:10 car, nothing in the reference fixes them
DEFAULTS = dict(margin=0.25, reach=0.5, half_length=0.4, half_width_car=0.2, restitution=0.2, friction=0.3, push=0.5, yaw_response=1)
F64_NAMES, I32_NAMES = _ffi.WALL_F64_NAMES, _ffi.WALL_I32_NAMES
CARRY_F64_NAMES, CARRY_I32_NAMES = _ffi.WALL_CARRY_F64_NAMES, _ffi.WALL_CARRY_I32_NAMES
# the corners' order: (sign of half_length, sign of half_width_car) of corner k
CORNER_SIGNS = ((1, 1), (1, -1), (-1, 1), (-1, -1))


def wall_config(**words):
    """An ``_ffi.WallConfig`` from the defaults and ``words`` (margin, reach, half_length, half_width_car, restitution, friction, push,
    yaw_response).  Raises ValueError for what lpvmpc_race_walls refuses: an unknown word, a word that is not finite, margin / friction
    < 0, reach / half_length / half_width_car not > 0, restitution / push outside [0, 1], yaw_response other than 0 / 1."""
    unknown = sorted(set(words) - set(DEFAULTS))
    if unknown:
        raise ValueError("wall_config: unknown word(s) %s (have %s)" % (unknown, sorted(DEFAULTS)))
    w = dict(DEFAULTS)
    w.update(words)
    y = w["yaw_response"]
    if isinstance(y, (bool, np.bool_)):
        y = int(y)
    if not isinstance(y, (int, np.integer)) or y not in (0, 1):
        raise ValueError("wall_config: yaw_response = %r must be 0 or 1" % (w["yaw_response"],))
    names = ("margin", "reach", "half_length", "half_width_car", "restitution", "friction", "push")
    for k in names:
        w[k] = float(w[k])
        if not math.isfinite(w[k]):
            raise ValueError("wall_config: %s = %g is not finite" % (k, w[k]))
    for k in ("margin", "friction"):
        if w[k] < 0.0:
            raise ValueError("wall_config: %s = %g must be >= 0" % (k, w[k]))
    for k in ("reach", "half_length", "half_width_car"):
        if not w[k] > 0.0:
            raise ValueError("wall_config: %s = %g must be > 0" % (k, w[k]))
    for k in ("restitution", "push"):
        if not 0.0 <= w[k] <= 1.0:
            raise ValueError("wall_config: %s = %g must lie in [0, 1]" % (k, w[k]))
    return _ffi.WallConfig(*([w[k] for k in names] + [int(y), 0]))


def as_config(cfg):
    """None (the defaults), a dict of words or an ``_ffi.WallConfig`` -> a checked ``_ffi.WallConfig``."""
    if cfg is None:
        return wall_config()
    if isinstance(cfg, dict):
        return wall_config(**cfg)
    if getattr(cfg, "reserved", 0) != 0:
        raise ValueError("wall_config: reserved = %r must be 0" % (cfg.reserved,))
    return wall_config(**{k: getattr(cfg, k) for k in DEFAULTS})


def new_carry(B):
    """The carried state "just attached" of ``BatchedSolver.wall_step`` for B vehicles: no impulse, no hit (first_hit_tick -1)."""
    return blank_carry(B, _ffi.WALL_CARRY_F64, CARRY_I32_NAMES, ("first_hit_tick",))


def walls_dict(f, i):
    """Output planes f [WALL_F64, B], i [WALL_I32, B] -> dict of [B] arrays named as _ffi.WALL_F64_NAMES / WALL_I32_NAMES and the planes
    themselves (f64, i32)."""
    return planes_dict(f, i, F64_NAMES, I32_NAMES)


def corners(plant, cfg=None):
    """The footprint corners [B, 4, 2] of plant rows [B, 8] (x, y, ..., yaw at word 6) in the header's order -- front left, front right,
    rear left, rear right -- and with its arithmetic: corner_k = (x + (c*a - s*b), y + (s*a + c*b)), (a, b) = (+-half_length,
    +-half_width_car).  ``cfg`` as ``wall_config`` (None: the defaults)."""
    c_ = as_config(cfg)
    p = np.asarray(plant, float)
    if p.ndim != 2 or p.shape[1] != 8:
        raise ValueError("corners: plant must be [B, 8], got %s" % (p.shape,))
    c, s = np.cos(p[:, 6]), np.sin(p[:, 6])
    out = np.empty((p.shape[0], 4, 2))
    for k, (sa, sb) in enumerate(CORNER_SIGNS):
        a, b = sa * c_.half_length, sb * c_.half_width_car
        out[:, k, 0] = p[:, 0] + (c * a - s * b)
        out[:, k, 1] = p[:, 1] + (s * a + c * b)
    return out
