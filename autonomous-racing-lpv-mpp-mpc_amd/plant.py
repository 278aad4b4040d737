"""Per-vehicle plant parameters for the device fleets and races (include/lpvmpc.h, "Per-vehicle plant parameters"): rows
[lf, lr, m, Iz, Cf, Cr, mu] per vehicle, with which each vehicle's simulated plant (Simulator.f, vehicleSimulator.py:164-199)
steps while the controllers, the planner and the estimator keep their nominal model.  Cf and Cr are the plant's linear tyre
stiffnesses (Simulator.f's constant 60), mu its drag coefficient (simulator/mu).  These helpers build and sample the rows; the
library checks them again."""
from __future__ import annotations

import numpy as np

from . import _ffi

WORDS = _ffi.PLANT_WORD_NAMES
NOMINAL = dict(lf=0.125, lr=0.125, m=1.98, Iz=0.03, Cf=60.0, Cr=60.0, mu=0.05)   # MAIN_LAUNCH.launch; Simulator.f's tyre; simulator/mu


def check_rows(rows, B, what="plant_params"):
    """The row check shared by the plant rows and the model rows (model.py): rows as a contiguous float64 [B, 7] array; ValueError
    naming ``what``, the vehicle and the field on another shape, a non-finite word, lf / lr / m / Iz <= 0 or Cf / Cr / mu < 0 (the
    library's refusals, raised before any call into it)."""
    a = np.asarray(rows)
    if a.dtype.kind not in "fiu":
        raise ValueError("%s must be numeric, got dtype %s" % (what, a.dtype))
    a = np.ascontiguousarray(a, np.float64)
    if a.shape != (B, _ffi.PLANT_WORDS):
        raise ValueError("%s has shape %s, expected (%d, %d) = (B, [lf lr m Iz Cf Cr mu])" % (what, a.shape, B, _ffi.PLANT_WORDS))
    if not np.all(np.isfinite(a)):
        b, i = np.argwhere(~np.isfinite(a))[0]
        raise ValueError("%s: vehicle %d: %s is not finite" % (what, b, WORDS[i]))
    bad = np.argwhere(np.concatenate([a[:, :4] <= 0, a[:, 4:] < 0], axis=1))
    if bad.size:
        b, i = bad[0]
        raise ValueError("%s: vehicle %d: %s = %g (lf, lr, m, Iz must be > 0; Cf, Cr, mu >= 0)" % (what, b, WORDS[i], a[b, i]))
    return a


def check_plant_params(rows, B):
    """rows as a contiguous float64 [B, 7] array; ValueError on another shape, a non-finite word, lf / lr / m / Iz <= 0 or
    Cf / Cr / mu < 0 (the library's refusals, raised before any call into it)."""
    return check_rows(rows, B, "plant_params")


def plant_params(B, engine=None, mu_sim=0.05, **fields):
    """[B, 7] nominal rows -- lf, lr, m, Iz of ``engine`` (a BatchedSolver; None: the launch file's), Cf = Cr = 60 (the simulator's
    tyre, not the controller's Cf) and mu = mu_sim -- with any field overridden by a scalar or a [B] array, e.g.
    plant_params(B, eng, m=np.linspace(1.7, 2.3, B))."""
    B = int(B)
    if B < 1:
        raise ValueError("B must be >= 1")
    base = dict(NOMINAL, mu=float(mu_sim))
    if engine is not None:
        base.update({k: float(getattr(engine.cfg, k)) for k in ("lf", "lr", "m", "Iz")})
    unknown = set(fields) - set(WORDS)
    if unknown:
        raise TypeError("unknown plant field(s) %s (fields: %s)" % (sorted(unknown), ", ".join(WORDS)))
    out = np.empty((B, _ffi.PLANT_WORDS))
    for i, k in enumerate(WORDS):
        v = np.asarray(fields.get(k, base[k]), np.float64)
        if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != B):
            raise ValueError("%s must be a scalar or have %d entries, got shape %s" % (k, B, v.shape))
        out[:, i] = v
    return check_plant_params(out, B)


# relative spread of each field for sample_plant_params: m, Iz +-15 %, Cf, Cr +-30 %, mu x [0.5, 1.5]
DEFAULT_SPREAD = dict(m=0.15, Iz=0.15, Cf=0.30, Cr=0.30, mu=0.50)


def sample_plant_params(B, seed, spread=None, engine=None, mu_sim=0.05, offset=0):
    """[B, 7] rows: each field of the nominal row (plant_params(B, engine, mu_sim)) times an independent uniform factor in
    [1 - s, 1 + s], s = spread[field] (dict; None: DEFAULT_SPREAD; fields not named stay nominal).  Seeded: vehicle b of a fleet
    gets the same row for the same seed whatever the batch, so shard k of a sharded fleet takes sample_plant_params(n, seed,
    offset=k * n) -- the rows of vehicles offset .. offset + n - 1 of one fleet."""
    B, offset = int(B), int(offset)
    spread = DEFAULT_SPREAD if spread is None else dict(spread)
    unknown = set(spread) - set(WORDS)
    if unknown:
        raise TypeError("unknown plant field(s) %s (fields: %s)" % (sorted(unknown), ", ".join(WORDS)))
    for k, s in spread.items():
        if not (np.isfinite(s) and 0 <= s < 1):
            raise ValueError("spread of %s must be in [0, 1), got %r" % (k, s))
    base = plant_params(B, engine, mu_sim)
    # one stream per (seed, field); a vehicle's factor is the stream's entry at its global index, so slices agree with the whole
    for i, k in enumerate(WORDS):
        if k in spread:
            u = np.random.default_rng([int(seed), i]).uniform(-1.0, 1.0, offset + B)[offset:]
            base[:, i] *= 1.0 + float(spread[k]) * u
    return check_plant_params(base, B)


# ---- tyre rows (include/lpvmpc.h, "Tyre model"): [kind, B, C, c_f] per vehicle -- kind 0 the linear tyre of the plant row, kind 1
# Simulator.pacejka (vehicleSimulator.py:202-205) on both axles
TYRE_WORDS = _ffi.TYRE_WORD_NAMES
PACEJKA = (1.0, 6.0, 1.6, 0.8)           # MAIN_LAUNCH.launch: simulator/B, simulator/C, simulator/c_f
DEFAULT_TYRE_SPREAD = dict(B=0.20, C=0.10, c_f=0.25)


def check_tyre_params(rows, B):
    """rows as a contiguous float64 [B, 4] array; ValueError on another shape, a kind other than exactly 0 or 1, or a non-finite or
    negative B, C, c_f (the library's refusals, raised before any call into it)."""
    a = np.asarray(rows)
    if a.dtype.kind not in "fiu":
        raise ValueError("tyre_params must be numeric, got dtype %s" % a.dtype)
    a = np.ascontiguousarray(a, np.float64)
    if a.shape != (B, _ffi.TYRE_WORDS):
        raise ValueError("tyre_params has shape %s, expected (%d, %d) = (B, [kind B C c_f])" % (a.shape, B, _ffi.TYRE_WORDS))
    bad = np.argwhere(np.concatenate([~np.isin(a[:, :1], (0.0, 1.0)), ~(np.isfinite(a[:, 1:]) & (a[:, 1:] >= 0))], axis=1))
    if bad.size:
        b, i = bad[0]
        raise ValueError("tyre_params: vehicle %d: %s = %g (kind must be 0 or 1; B, C, c_f finite and >= 0)" % (b, TYRE_WORDS[i], a[b, i]))
    return a


def tyre_params(B, kind=1, B_=PACEJKA[1], C=PACEJKA[2], c_f=PACEJKA[3]):
    """[B, 4] tyre rows [kind, B, C, c_f]: the launch file's Pacejka tyre by default, any word overridden by a scalar or a [B]
    array (the curve's B is spelt ``B_``), e.g. tyre_params(B, kind=np.arange(B) % 2) for an A/B inside one fleet."""
    B = int(B)
    if B < 1:
        raise ValueError("B must be >= 1")
    out = np.empty((B, _ffi.TYRE_WORDS))
    for i, (k, v) in enumerate(zip(TYRE_WORDS, (kind, B_, C, c_f))):
        v = np.asarray(v, np.float64)
        if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != B):
            raise ValueError("%s must be a scalar or have %d entries, got shape %s" % (k, B, v.shape))
        out[:, i] = v
    return check_tyre_params(out, B)


def pacejka(alpha, m, row=PACEJKA):
    """The lateral force of tyre row [kind, B, C, c_f] at slip angle alpha for a vehicle of mass m: Simulator.pacejka's
    D sin(C arctan(B alpha)), D = c_f m g / 2 in the reference's association (kind is not read: this is the curve)."""
    _, Bq, Cq, cf = (float(v) for v in row)
    D = cf * m * 9.81 / 2
    return D * np.sin(Cq * np.arctan(Bq * np.asarray(alpha, np.float64)))


def sample_tyre_params(B, seed, spread=None, kind=1, offset=0):
    """[B, 4] rows: the launch file's Pacejka words times independent uniform factors in [1 - s, 1 + s], s = spread[word] (dict over
    "B", "C", "c_f"; None: DEFAULT_TYRE_SPREAD), with ``kind`` (scalar or [B]) as given.  Seeded per vehicle like
    sample_plant_params: shard k of a sharded fleet takes sample_tyre_params(n, seed, offset=k * n)."""
    B, offset = int(B), int(offset)
    spread = DEFAULT_TYRE_SPREAD if spread is None else dict(spread)
    unknown = set(spread) - set(TYRE_WORDS[1:])
    if unknown:
        raise TypeError("unknown tyre word(s) %s (words: %s)" % (sorted(unknown), ", ".join(TYRE_WORDS[1:])))
    for k, s in spread.items():
        if not (np.isfinite(s) and 0 <= s < 1):
            raise ValueError("spread of %s must be in [0, 1), got %r" % (k, s))
    base = tyre_params(B, kind=kind)
    for i, k in enumerate(TYRE_WORDS):
        if k in spread:                   # (streams keyed apart from the plant rows': the third key word)
            u = np.random.default_rng([int(seed), i, 1]).uniform(-1.0, 1.0, offset + B)[offset:]
            base[:, i] *= 1.0 + float(spread[k]) * u
    return check_tyre_params(base, B)
