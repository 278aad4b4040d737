"""Contact model (include/lpvmpc.h, "Contact model"): host-side helpers of ``BatchedSolver.race_contact`` / ``race_contact_read`` /
``contact_step`` -- the configuration with the checks that need no device, the carried state of the batch form and the named views
of the two planes."""
from __future__ import annotations

import math

import numpy as np

from . import _ffi
from ._planes import blank_carry, planes_dict

# lpvmpc_contact_default_config: the walls' values
DEFAULTS = dict(friction=0.3, yaw_response=1)


def contact_config(**words):
    """An ``_ffi.ContactConfig`` from the defaults and ``words`` (friction, yaw_response).  Raises ValueError for what
    lpvmpc_race_contact refuses: an unknown word, friction not finite or < 0, yaw_response other than 0 / 1."""
    unknown = sorted(set(words) - set(DEFAULTS))
    if unknown:
        raise ValueError("contact_config: unknown word(s) %s (have %s)" % (unknown, sorted(DEFAULTS)))
    w = dict(DEFAULTS)
    w.update(words)
    y = w["yaw_response"]
    if isinstance(y, (bool, np.bool_)):
        y = int(y)
    if not isinstance(y, (int, np.integer)) or y not in (0, 1):
        raise ValueError("contact_config: yaw_response = %r must be 0 or 1" % (w["yaw_response"],))
    f = float(w["friction"])
    if not math.isfinite(f):
        raise ValueError("contact_config: friction = %g is not finite" % f)
    if f < 0.0:
        raise ValueError("contact_config: friction = %g must be >= 0" % f)
    return _ffi.ContactConfig(f, int(y), 0)


def as_config(cfg):
    """None (the defaults), a dict of words or an ``_ffi.ContactConfig`` -> a checked ``_ffi.ContactConfig``."""
    if cfg is None:
        return contact_config()
    if isinstance(cfg, dict):
        return contact_config(**cfg)
    return contact_config(**{k: getattr(cfg, k) for k in DEFAULTS})


def new_contact_carry(B):
    """The carried state "just attached" of ``BatchedSolver.contact_step`` for B vehicles: no yaw kick, no partner."""
    return blank_carry(B, _ffi.CONTACT_CARRY_F64, _ffi.CONTACT_CARRY_I32_NAMES)


def contact_dict(f, i):
    """Planes f [CONTACT_F64, B], i [CONTACT_I32, B] -> dict of [B] arrays named as _ffi.CONTACT_F64_NAMES / CONTACT_I32_NAMES and the
    planes themselves (f64, i32)."""
    return planes_dict(f, i, _ffi.CONTACT_F64_NAMES, _ffi.CONTACT_I32_NAMES)
