"""Tyre wear and temperature of a lap-0 fleet or a race (include/lpvmpc.h, "Tyre wear and temperature"): per vehicle a tyre-set state
(wear W, temperature T, sliding energy E) advanced at the control tick from the sliding power of the plant, and the grip factor g it
gives, which scales the plant's tyre stiffnesses and the Pacejka peak behind the disturbances' gamma.  Rows are [B, 12] =
WEAR_WORD_NAMES per vehicle, the state [B, 6] = WEAR_STATE_NAMES (BatchedSolver.set_tyre_wear, RaceFleet.wear)."""
import math

import numpy as np

from . import _ffi

WEAR_WORD_NAMES = ("k_wear", "k_hot", "k_heat", "k_cool", "T_amb", "T_opt", "k_temp", "wear_slope", "cliff_at", "cliff_slope", "g_min",
                   "T_start")
WEAR_STATE_NAMES = ("W", "T", "P", "g", "ticks", "E")
ALL_OFF = (0.0, 0.0, 0.0, 0.0, 20.0, 20.0, 0.0, 0.0, 1.0, 0.0, 1e-3, 20.0)
_NON_NEGATIVE = (0, 1, 2, 3, 6, 7, 9)


def check_tyre_wear_rows(rows, B, tick_s=None):
    """Validated float64 [B, 12] copy of ``rows`` with the library's refusals: every word finite; k_wear, k_hot, k_heat, k_cool,
    k_temp, wear_slope, cliff_slope >= 0; cliff_at in [0, 1]; g_min in (0, 1]; and -- with ``tick_s``, the longest control tick in
    seconds (n_max * dt_sim) -- k_cool * tick_s < 1, the bound of the temperature's Euler step."""
    a = np.asarray(rows)
    if a.dtype.kind not in "fiu":
        raise ValueError("tyre wear rows must be numeric, got dtype %s" % a.dtype)
    a = np.array(a, dtype=np.float64)
    if a.shape != (B, _ffi.WEAR_WORDS):
        raise ValueError("tyre wear rows have shape %s, expected (%d, %d) = (B, [%s])" % (a.shape, B, _ffi.WEAR_WORDS, " ".join(WEAR_WORD_NAMES)))
    for b in range(B):
        for i, v in enumerate(a[b]):
            ok = math.isfinite(v)
            if ok and i in _NON_NEGATIVE:
                ok = v >= 0
            elif ok and i == 8:
                ok = 0 <= v <= 1
            elif ok and i == 10:
                ok = 0 < v <= 1
            if not ok:
                raise ValueError("tyre wear rows: vehicle %d: %s = %g (every word finite; k_wear, k_hot, k_heat, k_cool, k_temp, wear_slope, "
                                 "cliff_slope >= 0; cliff_at in [0, 1]; g_min in (0, 1])" % (b, WEAR_WORD_NAMES[i], v))
        if tick_s is not None and not a[b, 3] * float(tick_s) < 1.0:
            raise ValueError("tyre wear rows: vehicle %d: k_cool * tick = %g * %g >= 1 (the temperature's Euler step would overshoot the "
                             "ambient)" % (b, a[b, 3], tick_s))
    return np.ascontiguousarray(a)


def tyre_wear_rows(B, tick_s=None, **words):
    """[B, 12] rows, all off (every k_ and slope 0, cliff_at 1, g_min 1e-3, T_amb = T_opt = T_start = 20: g stays 1 and T stays
    T_start) with any word of WEAR_WORD_NAMES overridden by a scalar or a [B] array."""
    out = np.tile(np.array(ALL_OFF), (B, 1))
    unknown = set(words) - set(WEAR_WORD_NAMES)
    if unknown:
        raise TypeError("unknown tyre wear word(s) %s (words: %s)" % (sorted(unknown), ", ".join(WEAR_WORD_NAMES)))
    for k, v in words.items():
        out[:, WEAR_WORD_NAMES.index(k)] = np.broadcast_to(np.asarray(v, float), (B,))
    return check_tyre_wear_rows(out, B, tick_s)


def sample_tyre_wear(B, seed, spread=None, tick_s=None, offset=0):
    """Monte-Carlo rows: word w of vehicle b is uniform in ``spread[w] = (lo, hi)`` (a word not in ``spread`` stays off), drawn from a
    generator keyed (seed, offset + b) so that shard k of a sharded fleet takes sample_tyre_wear(n, seed, offset=k * n).  Default
    spread: a set that wears to its cliff within some thousand joules of sliding, warms by some ten degrees and cools within seconds."""
    spread = dict(k_wear=(2e-4, 1e-3), k_hot=(0.0, 0.05), k_heat=(0.5, 2.0), k_cool=(0.2, 1.0), T_opt=(25.0, 40.0), k_temp=(1e-4, 5e-4),
                  wear_slope=(0.05, 0.2), cliff_at=(0.6, 0.9), cliff_slope=(1.0, 3.0), g_min=(0.2, 0.5)) if spread is None else dict(spread)
    unknown = set(spread) - set(WEAR_WORD_NAMES)
    if unknown:
        raise TypeError("unknown tyre wear word(s) %s (words: %s)" % (sorted(unknown), ", ".join(WEAR_WORD_NAMES)))
    out = np.tile(np.array(ALL_OFF), (B, 1))
    for b in range(B):
        rng = np.random.default_rng([int(seed), int(offset) + b])
        u = rng.random(_ffi.WEAR_WORDS)
        for k, (lo, hi) in spread.items():
            i = WEAR_WORD_NAMES.index(k)
            out[b, i] = lo + (hi - lo) * u[i]
    return check_tyre_wear_rows(out, B, tick_s)
