"""Per-vehicle tunings (include/lpvmpc.h, "Per-vehicle tunings"): rows of 64 words -- Q, R, dR, L_cf and the box limits -- with
which a controller or planner engine builds the QP of each instance of a batch -- each vehicle of a fleet, cascade or race --
instead of the one tuning of its configuration (BatchedSolver.set_tunings; RaceFleet(path_tunings=, tt_tunings=, plan_tunings=)).
A row is in the units of the engine's constructor arguments:

    [0:36]  Q, nx*nx row-major in the first nx*nx slots      [36:40] R      [40:42] dR      [42:48] L_cf (planner)
    [48:64] limits.  Controller: vx_min, max_vel, delta_max, a_max, a_min_abs.  Planner: xmin[5], xmax[5], umin[2], umax[2]
            (xmin[0] / xmax[0] are min_vel / max_vel; slot 3, ey, is ignored: max_ey stays a per-instance argument).

These helpers build and sample the rows; the library checks them again."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi

WORDS = _ffi.TUNING_WORDS
Q0, R0, DR0, LCF0, LIM0 = 0, 36, 40, 42, 48
CTRL_LIMITS = ("vx_min", "max_vel", "delta_max", "a_max", "a_min_abs")           # words 48 ..
PLAN_LIMITS = (("xmin", 48, 5), ("xmax", 53, 5), ("umin", 58, 2), ("umax", 60, 2))
# sample_tunings' default: every diagonal weight +-30 %; the limits stay the engine's
DEFAULT_SPREAD = {"Q": 0.3, "R": 0.3, "dR": 0.3, "L_cf": 0.3}


def _kind(engine):
    """(kind, nx) of an engine (BatchedSolver), or of the strings "controller" / "planner" / a KIND_* value."""
    k = getattr(engine, "kind", engine)
    k = {"controller": _ffi.KIND_CONTROLLER, "planner": _ffi.KIND_PLANNER}.get(k, k)
    if k not in (_ffi.KIND_CONTROLLER, _ffi.KIND_PLANNER):
        raise ValueError("engine must be a BatchedSolver, 'controller' or 'planner', got %r" % (engine,))
    return k, (6 if k == _ffi.KIND_CONTROLLER else 5)


def fields(kind):
    """name -> (first word, shape) of the fields of a row of this kind that the solve reads."""
    kind, nx = _kind(kind)
    f = {"Q": (Q0, (nx, nx)), "R": (R0, (2, 2)), "dR": (DR0, (2,))}
    if kind == _ffi.KIND_CONTROLLER:
        for i, k in enumerate(CTRL_LIMITS):
            f[k] = (LIM0 + i, ())
    else:
        f["L_cf"] = (LCF0, (5,))
        for k, w, n in PLAN_LIMITS:
            f[k] = (w, (n,))
    return f


def check_tuning_rows(rows, B, kind):
    """rows as a contiguous float64 [B, 64] array; ValueError naming instance and field on another shape, a non-finite weight, a
    NaN limit or a lower limit above its upper one (the library's refusals, raised before any call into it)."""
    kind, nx = _kind(kind)
    a = np.ascontiguousarray(rows, np.float64)
    if a.ndim != 2 or a.shape != (int(B), WORDS):
        raise ValueError("tunings has shape %s, expected (%d, %d)" % (a.shape, int(B), WORDS))
    f = fields(kind)

    def first_bad(mask, what):
        if mask.any():
            raise ValueError("tunings: instance %d: %s" % (int(np.argmax(mask.reshape(a.shape[0], -1).any(axis=1))), what))

    for k in ("Q", "R", "dR") + (("L_cf",) if kind == _ffi.KIND_PLANNER else ()):
        w, shp = f[k]
        first_bad(~np.isfinite(a[:, w:w + int(np.prod(shp))]), "a non-finite word of %s" % k)
    lim = a[:, LIM0:]
    if kind == _ffi.KIND_CONTROLLER:
        first_bad(np.isnan(lim[:, :5]), "a NaN limit")
        first_bad(lim[:, 0] > lim[:, 1], "vx_min > max_vel")
        first_bad(lim[:, 2] < 0, "delta_max < 0")
        first_bad(lim[:, 3] < -lim[:, 4], "a_max < -a_min_abs")
    else:
        used = [0, 1, 2, 4]
        first_bad(np.isnan(lim[:, used + [5 + r for r in used] + [10, 11, 12, 13]]), "a NaN limit")
        first_bad(lim[:, used] > lim[:, [5 + r for r in used]], "xmin > xmax")
        first_bad(lim[:, 10:12] > lim[:, 12:14], "umin > umax")
    return a


def config_row(cfg):
    """The row a handle created from the lpvmpc_config ``cfg`` solves with (lpvmpc_tuning_from_config; host only)."""
    row = np.zeros(WORDS)
    rc = _ffi.load().lpvmpc_tuning_from_config(C.byref(cfg), _ffi.ptr(row))
    if rc:
        raise ValueError("lpvmpc_tuning_from_config failed (%d)" % rc)
    return row


def device_row(kind, row):
    """The 64 words the solve kernel reads for a public row: Q R dR Lcf box_lo[8] box_hi[8] (lpvmpc_tuning_device_row; host only)."""
    kind, _ = _kind(kind)
    row = np.ascontiguousarray(row, np.float64)
    if row.shape != (WORDS,):
        raise ValueError("row has shape %s, expected (%d,)" % (row.shape, WORDS))
    out = np.zeros(WORDS)
    rc = _ffi.load().lpvmpc_tuning_device_row(int(kind), _ffi.ptr(row), _ffi.ptr(out))
    if rc:
        raise ValueError("lpvmpc_tuning_device_row failed (%d)" % rc)
    return out


def tuning_rows(B, engine, **overrides):
    """[B, 64] rows of the tuning ``engine`` (a BatchedSolver) solves with today, with any field overridden by one value for all
    instances or one per instance: Q [nx, nx] or [B, nx, nx], R [2, 2] or [B, 2, 2], dR [2] or [B, 2]; controller: vx_min, max_vel,
    delta_max, a_max, a_min_abs as scalars or [B]; planner: L_cf [5] or [B, 5], xmin / xmax [5] or [B, 5], umin / umax [2] or [B, 2],
    e.g. tuning_rows(B, eng, delta_max=np.linspace(0.15, 0.249, B))."""
    B = int(B)
    if B < 1:
        raise ValueError("B must be >= 1")
    kind, _ = _kind(engine)
    f = fields(kind)
    unknown = set(overrides) - set(f)
    if unknown:
        raise TypeError("unknown tuning field(s) %s (fields: %s)" % (sorted(unknown), ", ".join(f)))
    out = np.tile(config_row(engine.cfg), (B, 1))
    for k, v in overrides.items():
        w, shp = f[k]
        v = np.asarray(v, np.float64)
        if v.shape == shp:
            v = np.broadcast_to(v, (B,) + shp)
        elif v.shape != (B,) + shp:
            raise ValueError("%s must have shape %s or %s, got %s" % (k, shp, (B,) + shp, v.shape))
        out[:, w:w + int(np.prod(shp, dtype=int))] = v.reshape(B, -1)
    return check_tuning_rows(out, B, kind)


def perturb_rows(rows, kind, seed, spread, offset=0):
    """rows [B, 64] with each field named in ``spread`` (dict field -> s, 0 <= s < 1) times independent uniform factors in
    [1 - s, 1 + s]: one factor per diagonal entry of Q and R (off-diagonal entries stay as they are), one per entry of dR, L_cf and
    of a limit field.  Seeded per (seed, field) and per GLOBAL vehicle index offset + b, so slices agree with the whole."""
    kind, nx = _kind(kind)
    a = np.array(rows, np.float64)
    B, offset = a.shape[0], int(offset)
    f = fields(kind)
    unknown = set(spread) - set(f)
    if unknown:
        raise TypeError("unknown tuning field(s) %s (fields: %s)" % (sorted(unknown), ", ".join(f)))
    for k, s in spread.items():
        if not (np.isfinite(s) and 0 <= s < 1):
            raise ValueError("spread of %s must be in [0, 1), got %r" % (k, s))
    for i, k in enumerate(f):
        if k not in spread:
            continue
        w, shp = f[k]
        n = shp[0] if shp else 1
        u = np.random.default_rng([int(seed), i, 2]).uniform(-1.0, 1.0, (offset + B, n))[offset:]
        cols = [w + j * (shp[1] + 1) for j in range(n)] if len(shp) == 2 else list(range(w, w + n))
        a[:, cols] *= 1.0 + float(spread[k]) * u
    return check_tuning_rows(a, B, kind)


def sample_tunings(B, seed, spread=None, engine=None, offset=0):
    """[B, 64] rows: the engine's own tuning (tuning_rows(B, engine)) with each field named in ``spread`` scaled by independent
    uniform factors in [1 - s, 1 + s] (dict; None: DEFAULT_SPREAD, every diagonal weight +-30 %; fields not named stay the
    engine's).  Seeded like model.sample_model_params: vehicle b of a fleet gets the same row for the same seed whatever the batch,
    so shard k of a sharded fleet takes sample_tunings(n, seed, engine=eng, offset=k * n)."""
    if engine is None:
        raise ValueError("sample_tunings needs the engine whose tuning it varies")
    kind, _ = _kind(engine)
    spread = {k: v for k, v in DEFAULT_SPREAD.items() if k in fields(kind)} if spread is None else dict(spread)
    return perturb_rows(tuning_rows(int(B), engine), kind, seed, spread, offset)


def split_row(kind, row):
    """A row's fields as a dict of arrays (Q [nx, nx], R [2, 2], ...): the constructor arguments of the plain engine of that tuning."""
    row = np.asarray(row, np.float64)
    return {k: (row[w:w + int(np.prod(shp, dtype=int))].reshape(shp).copy() if shp else float(row[w])) for k, (w, shp) in fields(kind).items()}


def engine_kwargs(kind, row):
    """split_row as keyword arguments of BatchedSolver(kind, N, dt, **kw): the plain engine that solves every instance with this row."""
    kind, _ = _kind(kind)
    d = split_row(kind, row)
    kw = {"Q": d["Q"], "R": d["R"], "dR": d["dR"]}
    if kind == _ffi.KIND_CONTROLLER:
        kw.update(ctrl_vx_min=d["vx_min"], ctrl_delta_max=d["delta_max"], ctrl_a_max=d["a_max"], ctrl_a_min_abs=d["a_min_abs"])
        kw["params"] = {"max_vel": d["max_vel"]}
    else:
        kw.update(L_cf=d["L_cf"], plan_xmin=d["xmin"], plan_xmax=d["xmax"], plan_umin=d["umin"], plan_umax=d["umax"])
        kw["params"] = {"min_vel": d["xmin"][0], "max_vel": d["xmax"][0]}
    return kw
