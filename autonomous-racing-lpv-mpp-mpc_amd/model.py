"""Per-vehicle model parameters (include/lpvmpc.h, "Per-vehicle model parameters"): rows [lf, lr, m, Iz, Cf, Cr, mu] per vehicle
with which a controller or planner engine linearises each instance of a batch -- each vehicle of a fleet, cascade or race --
instead of the one vehicle of its configuration (BatchedSolver.set_model_params; RaceFleet(model_params=...)).  The word order is
the plant rows' (plant.py), so a vehicle's plant row can be bound as its model: the matched experiment.  Unlike a plant row, whose
Cf = Cr = 60 is the simulator's tyre, a model row's nominal words are the engine's own (its Cf, Cr and mu).  In the controller
roll-out the row's Cf stands for both axles and the call's cf_new is ignored.  These helpers build and sample the rows; the
library checks them again."""
from __future__ import annotations

import numpy as np

from . import _ffi
from .plant import DEFAULT_SPREAD, NOMINAL, WORDS, check_rows


def check_model_params(rows, B):
    """rows as a contiguous float64 [B, 7] array; ValueError naming vehicle and field on another shape, a non-finite word,
    lf / lr / m / Iz <= 0 or Cf / Cr / mu < 0 (plant.check_rows: the library's refusals, raised before any call into it)."""
    return check_rows(rows, B, "model_params")


def model_params(B, engine=None, **fields):
    """[B, 7] rows of the words ``engine`` (a BatchedSolver; None: the launch file's vehicle) linearises with today, with any field
    overridden by a scalar or a [B] array, e.g. model_params(B, eng, m=np.linspace(1.7, 2.3, B))."""
    B = int(B)
    if B < 1:
        raise ValueError("B must be >= 1")
    base = dict(NOMINAL)
    if engine is not None:
        base = {k: float(getattr(engine.cfg, k)) for k in WORDS}
    unknown = set(fields) - set(WORDS)
    if unknown:
        raise TypeError("unknown model field(s) %s (fields: %s)" % (sorted(unknown), ", ".join(WORDS)))
    out = np.empty((B, _ffi.MODEL_WORDS))
    for i, k in enumerate(WORDS):
        v = np.asarray(fields.get(k, base[k]), np.float64)
        if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != B):
            raise ValueError("%s must be a scalar or have %d entries, got shape %s" % (k, B, v.shape))
        out[:, i] = v
    return check_model_params(out, B)


def perturb_rows(rows, seed, spread, offset=0):
    """rows [B, 7] with each field named in ``spread`` (dict field -> s, 0 <= s < 1) times an independent uniform factor in
    [1 - s, 1 + s].  Seeded per (seed, field) and per GLOBAL vehicle index offset + b, so slices agree with the whole; the streams
    are not those of plant.sample_plant_params, so a model error drawn here is independent of a plant sampled with the same seed."""
    a = np.array(rows, np.float64)
    B, offset = a.shape[0], int(offset)
    unknown = set(spread) - set(WORDS)
    if unknown:
        raise TypeError("unknown model field(s) %s (fields: %s)" % (sorted(unknown), ", ".join(WORDS)))
    for k, s in spread.items():
        if not (np.isfinite(s) and 0 <= s < 1):
            raise ValueError("spread of %s must be in [0, 1), got %r" % (k, s))
    for i, k in enumerate(WORDS):
        if k in spread:
            u = np.random.default_rng([int(seed), i, 1]).uniform(-1.0, 1.0, offset + B)[offset:]
            a[:, i] *= 1.0 + float(spread[k]) * u
    return check_model_params(a, B)


def sample_model_params(B, seed, spread=None, engine=None, offset=0):
    """[B, 7] rows: each field of the engine's row (model_params(B, engine)) times an independent uniform factor in [1 - s, 1 + s],
    s = spread[field] (dict; None: plant.DEFAULT_SPREAD = m, Iz +-15 %, Cf, Cr +-30 %, mu x [0.5, 1.5]; fields not named stay
    nominal).  Seeded like plant.sample_plant_params: vehicle b of a fleet gets the same row for the same seed whatever the batch, so
    shard k of a sharded fleet takes sample_model_params(n, seed, offset=k * n)."""
    spread = DEFAULT_SPREAD if spread is None else dict(spread)
    return perturb_rows(model_params(int(B), engine), seed, spread, offset)
