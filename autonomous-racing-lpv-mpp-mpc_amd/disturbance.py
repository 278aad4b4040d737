"""Plant disturbances of a lap-0 fleet or a race (include/lpvmpc.h, "Plant disturbances"): per vehicle a first-order Gauss-Markov
gust on ax, ay and the yaw acceleration, one kick (vy, psiDot) at a plant step, and two low-grip patches along the lap that scale
the plant's tyre stiffnesses and the Pacejka peak.  Rows are [B, 13] = DIST_WORD_NAMES per vehicle; the model acts at the control
tick, in front of the tick's plant steps (BatchedSolver.set_disturbances, RaceFleet(disturbance=...))."""
import math

import numpy as np

from . import _ffi

DIST_WORD_NAMES = ("sigma_ax", "sigma_ay", "sigma_aw", "rho", "kick_step", "kick_vy", "kick_w",
                   "p0_s0", "p0_len", "p0_gamma", "p1_s0", "p1_len", "p1_gamma")
DIST_STATE_NAMES = ("d_ax", "d_ay", "d_aw", "ticks", "gamma")
ALL_OFF = (0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0)


def rho_from_tau(tau, tick_s):
    """The per-tick correlation of a gust with correlation time ``tau`` seconds at a control tick of ``tick_s`` seconds:
    exp(-tick_s / tau); tau = 0 gives white noise (rho = 0)."""
    if tau < 0 or tick_s <= 0:
        raise ValueError("rho_from_tau: tau >= 0 and tick_s > 0, got %r, %r" % (tau, tick_s))
    return 0.0 if tau == 0 else math.exp(-float(tick_s) / float(tau))


def check_disturbance_rows(rows, B, lap_length=None):
    """Validated float64 [B, 13] copy of ``rows`` with the library's refusals: every word finite, sigma >= 0, rho in [0, 1),
    kick_step integer-valued and < 2^31, gamma >= 0, s0 >= 0, len >= 0 and -- with ``lap_length`` (a scalar or [B], each vehicle's
    track) -- s0 < L, len <= L."""
    a = np.asarray(rows)
    if a.dtype.kind not in "fiu":
        raise ValueError("disturbance rows must be numeric, got dtype %s" % a.dtype)
    a = np.array(a, dtype=np.float64)
    if a.shape != (B, _ffi.DIST_WORDS):
        raise ValueError("disturbance rows have shape %s, expected (%d, %d) = (B, [%s])" % (a.shape, B, _ffi.DIST_WORDS, " ".join(DIST_WORD_NAMES)))
    L = None if lap_length is None else np.broadcast_to(np.asarray(lap_length, float), (B,))
    for b in range(B):
        for i, v in enumerate(a[b]):
            ok = math.isfinite(v)
            if ok and i < 3:
                ok = v >= 0
            elif ok and i == 3:
                ok = 0 <= v < 1
            elif ok and i == 4:
                ok = v == math.floor(v) and v < 2.0 ** 31
            elif ok and i in (7, 10):
                ok = v >= 0 and (L is None or v < L[b])
            elif ok and i in (8, 11):
                ok = v >= 0 and (L is None or v <= L[b])
            elif ok and i in (9, 12):
                ok = v >= 0
            if not ok:
                raise ValueError("disturbance rows: vehicle %d: %s = %g (every word finite; sigma >= 0; rho in [0, 1); kick_step "
                                 "integer-valued and < 2^31; 0 <= s0 < L; 0 <= len <= L; gamma >= 0)" % (b, DIST_WORD_NAMES[i], v))
    return np.ascontiguousarray(a)


def disturbance_rows(B, lap_length=None, **words):
    """[B, 13] rows, all off (sigma 0, kick_step -1, len 0, gamma 1) with any word of DIST_WORD_NAMES overridden by a scalar or a [B]
    array; ``sigma`` sets the three gust channels at once, ``patch0`` / ``patch1`` = (s0, len, gamma) a whole patch, ``kick`` =
    (step, vy, w) the kick."""
    out = np.tile(np.array(ALL_OFF), (B, 1))
    words = dict(words)
    if "sigma" in words:
        s = words.pop("sigma")
        for k in ("sigma_ax", "sigma_ay", "sigma_aw"):
            words.setdefault(k, s)
    for p in (0, 1):
        if "patch%d" % p in words:
            v = words.pop("patch%d" % p)
            for k, x in zip(("s0", "len", "gamma"), v):
                words["p%d_%s" % (p, k)] = x
    if "kick" in words:
        for k, x in zip(("kick_step", "kick_vy", "kick_w"), words.pop("kick")):
            words[k] = x
    unknown = set(words) - set(DIST_WORD_NAMES)
    if unknown:
        raise TypeError("unknown disturbance word(s) %s (words: %s, sigma, patch0, patch1, kick)" % (sorted(unknown), ", ".join(DIST_WORD_NAMES)))
    for k, v in words.items():
        out[:, DIST_WORD_NAMES.index(k)] = np.broadcast_to(np.asarray(v, float), (B,))
    return check_disturbance_rows(out, B, lap_length)


def sample_disturbances(B, seed, spread=None, lap_length=None, offset=0):
    """Monte-Carlo rows: word w of vehicle b is uniform in ``spread[w] = (lo, hi)`` (a word not in ``spread`` stays off), drawn from
    a generator keyed (seed, offset + b) so that shard k of a sharded fleet takes sample_disturbances(n, seed, offset=k * n);
    kick_step is rounded down to an integer.  Default spread: gusts of 0.2 .. 1.0 m/s^2 (rad/s^2 on the yaw channel), rho 0.5 .. 0.95."""
    spread = dict(sigma_ax=(0.2, 1.0), sigma_ay=(0.2, 1.0), sigma_aw=(0.2, 1.0), rho=(0.5, 0.95)) if spread is None else dict(spread)
    unknown = set(spread) - set(DIST_WORD_NAMES)
    if unknown:
        raise TypeError("unknown disturbance word(s) %s (words: %s)" % (sorted(unknown), ", ".join(DIST_WORD_NAMES)))
    out = np.tile(np.array(ALL_OFF), (B, 1))
    for b in range(B):
        rng = np.random.default_rng([int(seed), int(offset) + b])
        u = rng.random(_ffi.DIST_WORDS)
        for k, (lo, hi) in spread.items():
            i = DIST_WORD_NAMES.index(k)
            v = lo + (hi - lo) * u[i]
            out[b, i] = math.floor(v) if k == "kick_step" else v
    return check_disturbance_rows(out, B, lap_length)


def disturbance_config(seed=0, vehicle_offset=0, n_bound=None):
    """A ``lpvmpc_disturbance_config`` (the library's defaults with the given fields)."""
    c = _ffi.default_disturbance_config()
    c.seed = int(seed) & ((1 << 64) - 1); c.vehicle_offset = int(vehicle_offset)
    if n_bound is not None:
        c.n_bound = float(n_bound)
    return c


def parse_disturbance(spec, B, lap_length=None, rho=0.8):
    """Rows for the command-line tools' ``--disturbance`` flag, the same for every vehicle: ``gusts:SIGMA`` (the three channels, per-tick
    correlation ``rho``), ``patch:S0,LEN,GAMMA`` or ``kick:STEP,VY,W``; several may be joined with ``+``."""
    words = {}
    for part in str(spec).split("+"):
        kind, _, arg = part.partition(":")
        try:
            v = [float(x) for x in arg.split(",")]
        except ValueError:
            v = []
        if kind == "gusts" and len(v) == 1:
            words.update(sigma=v[0], rho=rho)
        elif kind == "patch" and len(v) == 3:
            words["patch1" if "patch0" in words else "patch0"] = v
        elif kind == "kick" and len(v) == 3:
            words["kick"] = v
        else:
            raise ValueError("--disturbance takes gusts:SIGMA, patch:S0,LEN,GAMMA or kick:STEP,VY,W (joined with +), got %r" % (part,))
    return disturbance_rows(B, lap_length, **words)
