"""Shared by tests/test_track_edges_host.py, tests/test_gpu_track_edges.py and tests/golden/track_edges/: the edge grid of the track
geometry (seams, lap ends, closing rows, width limit, headings turns away from the tangent), the float64-exact lookup rules and a
numpy.longdouble restatement of getLocalPosition / getGlobalPosition that knows how far every decision it takes is from flipping.

THE GRID is deterministic (one seeded draw, HEADING_SEED, picks the second heading of the lap-ahead points).  Tracks: the six of
track.palette() plus two Map.from_segments tracks, `full` (LPVMPC_MAX_TRACK_ROWS rows, left and right arcs, a 5 mm segment) and
`right` (right-hand arcs only).
  s       for every seam (every row's start, and the lap end L): seam + ds, ds in DS = {0, one ulp down, one ulp up, +-1e-9, +-1e-6,
          +-1e-3}; the same s one and two laps ahead (s + L, s + L + L in float64); and the specials -0.0, nextafter(0, -1), -1e-3,
          4096 L, nextafter(4096 L, inf), inf, nan.
  ey      {0, +-hw/2, +-(hw + slack)(1 - 1e-9), +-(hw + slack)(1 + 1e-9), +-2 (hw + slack)}.
  global  every (s, ey).
  local   (x, y, theta) of oracle/plant_ref.py's get_global_position at every (s, ey) where it answers, with heading theta + dpsi;
          every row's end point, word for word from the table (the norm == 0 branches); and, on every straight, the two points at
          mid length exactly hw + slack (the float64 sum) off the centre line.
  dpsi    DPSI = {0, +-0.3, +-pi, +-nextafter(pi, 0), 3.5, +-(2 pi k + 0.1) for k in (1, 3), 1000}.
Which heading goes with which point is chosen so that the cap of tests/test_track_edges_host.py on the undecided share holds (at
most 5 %).  A point 0 or one ulp from a seam with ey != 0 is undecided by construction (the angle that separates two rows is within
1e-14 of pi / 2), and so is any heading half a turn from the tangent: they are a third of the points and 4 of 13 headings.  So
  * a point with |ds| >= 1e-9 on the lap itself gets every dpsi that is not half a turn (nine headings),
  * its copies one and two laps ahead get dpsi = 0 and a second heading picked by the seeded draw,
  * a point with |ds| <= one ulp gets dpsi = 0, and its copies laps ahead are left to the global grid (the addition of L rounds
    the ulp away: they are the same point again),
  * a row's end point gets all thirteen, and the points at seams 1, 2, 3 + 1e-3, ey = 0 the four half turns as well.

THE RULES.  lookup_row is the segment selection of global_position and track_curvature: float64 statements, never "undecided".
THE RESTATEMENT.  locate / global_ld evaluate the reference's statements in numpy.longdouble on the float64 words as exact numbers,
with the float64 constant numpy.pi wherever the reference writes np.pi, and the float64 sum hw + slack.  Every comparison that
selects a branch records its margin; a case is DECIDED when every margin is at least TAU.  An undecided case is re-run with each
under-margin decision forced either way: the set of results is the expectation.  Two notes on the margins:
  * the unwrap margin is taken on the accepting row only: the epsi a rejected straight row computes is overwritten before it can
    be returned (an accepting row always writes its own), so that value reaches no output;
  * arctan2 has its own edge at +-pi, where sign(arc2) flips: the sign decision's margin is min(|arc2|, pi - |arc2|).
"""
import numpy as np

from oracle import plant_ref as PR

LD = np.longdouble
PI = LD(np.pi)                       # the reference's np.pi, the device's kPi: that double, exactly
TAU = 1e-12                          # rad or m: a few hundred rounded float64 operations at 20 m (4.4e-15 each), 1000 x below 1e-9
MAX_VARIANTS = 8
MAX_WRAP_LAPS = 4096                 # kMaxWrapLaps (csrc/lpvmpc_device.hpp)
HEADING_SEED = 20261

# measured by tests/test_track_edges_host.py::test_restatement_against_the_oracle on the decided grid (docs/HISTORY.md):
# worst |float64 oracle - long double restatement|
# -- separately for the local position (s, ey), the local heading error epsi (whose worst case is a heading of 1000 rad, where one
# ulp is 1.1e-13) and the global pose (x, y, theta)
ORACLE_DEV_LOCAL = 4.9e-15
ORACLE_DEV_EPSI = 2.8e-14
ORACLE_DEV_GLOBAL = 3.1e-15
# the GPU tests' bounds on decided coordinates: 100 x the measured deviation of that quantity, never above the project's 1e-11
GPU_BOUND_LOCAL = min(100.0 * ORACLE_DEV_LOCAL, 1e-11)
GPU_BOUND_EPSI = min(100.0 * ORACLE_DEV_EPSI, 1e-11)
GPU_BOUND_GLOBAL = min(100.0 * ORACLE_DEV_GLOBAL, 1e-11)
LOCAL_BOUNDS = (GPU_BOUND_LOCAL, GPU_BOUND_LOCAL, GPU_BOUND_EPSI)          # per column of (s, ey, epsi)

_PI64 = float(np.pi)
DS = (0.0, "down", "up", -1e-9, 1e-9, -1e-6, 1e-6, -1e-3, 1e-3)
DPSI = (0.0, 0.3, -0.3, 3.5, 2 * _PI64 + 0.1, -(2 * _PI64 + 0.1), 6 * _PI64 + 0.1, -(6 * _PI64 + 0.1), 1000.0,
        _PI64, -_PI64, float(np.nextafter(_PI64, 0.0)), -float(np.nextafter(_PI64, 0.0)))
N_PLAIN = 9                          # DPSI[:9] are not half a turn
REFERENCE_SHAPES = ("oval", "L_shape", "3110", "Euge_Track")      # palette entries 0 .. 3


def tracks():
    """The eight maps of the grid: track.palette() plus `full` and `right`."""
    from lpvmpc import track as T
    r = 4.5 / _PI64
    full = T.Map.from_segments([(0.5, 0), (0.005, 0), (0.495, 0), (1.5, r), (1.5, r), (1.5, r), (0.2, 0), (0.6, -1.5), (1.2, 1.5),
                                (0.6, -1.5), (1.5, r), (1.5, r), (1.5, r), (0.7, 0), (0.2, 0)], 0.3, 0.15, shape="full")
    assert full.PointAndTangent.shape[0] == T.MAX_TRACK_ROWS
    rr = 3.6 / _PI64
    right = T.Map.from_segments([(0.8, 0), (3.6, -rr), (1.6, 0), (3.6, -rr), (0.8, 0)], 0.25, 0.1, shape="right")
    return T.palette() + [full, right]


def lap_length(tab):
    return float(tab[-1, 3] + tab[-1, 4])


def seams(tab):
    return np.append(tab[:, 3], lap_length(tab))


def _offset(seam, ds):
    if ds == "down":
        return float(np.nextafter(seam, -np.inf))
    if ds == "up":
        return float(np.nextafter(seam, np.inf))
    return float(seam + ds)


def s_grid(tab):
    """s [n], seam index [n] (-1: a special), DS index [n], laps ahead [n]."""
    L = lap_length(tab)
    s, j_, d_, lap = [], [], [], []
    for j, seam in enumerate(seams(tab)):
        for d, ds in enumerate(DS):
            v = _offset(seam, ds)
            for k, w in enumerate((v, v + L, v + L + L)):
                s.append(w); j_.append(j); d_.append(d); lap.append(k)
    top = float(MAX_WRAP_LAPS * L)
    for v in (-0.0, float(np.nextafter(0.0, -1.0)), -1e-3, top, float(np.nextafter(top, np.inf)), np.inf, np.nan):
        s.append(v); j_.append(-1); d_.append(-1); lap.append(0)
    return np.array(s), np.array(j_, np.int32), np.array(d_, np.int32), np.array(lap, np.int32)


def ey_grid(m):
    w = float(m.halfWidth) + float(m.slack)
    return np.array([0.0, m.halfWidth / 2, -m.halfWidth / 2, w * (1 - 1e-9), -w * (1 - 1e-9), w * (1 + 1e-9), -w * (1 + 1e-9), 2 * w, -2 * w])


# ---- the float64-exact rules ----------------------------------------------------------------------------------------------------
def wrap_s(tab, s):
    """The reference's repeated subtraction in float64; NaN beyond kMaxWrapLaps laps and for a non-finite s."""
    L = np.float64(lap_length(tab))
    s = np.float64(s)
    if not (s <= L * np.float64(MAX_WRAP_LAPS)):
        return np.float64(np.nan)
    while s > L:
        s = s - L
    return s


def lookup_row(tab, s):
    """(row, wrapped s): the first row with s >= start and s < start + len in float64 after wrap_s; row -1 where none qualifies."""
    w = wrap_s(tab, s)
    for i in range(tab.shape[0]):
        if w >= tab[i, 3] and w < tab[i, 3] + tab[i, 4]:
            return i, w
    return -1, w


def curvature_rule(tab, s):
    i = lookup_row(tab, s)[0]
    return float(tab[i, 5]) if i >= 0 else float("nan")


# ---- the long double restatement -------------------------------------------------------------------------------------------------
def _sgn(a):
    return 1 if a >= 0 else -1


def _wrap_ld(a):
    if a < -PI:
        return 2 * PI + a
    if a > PI:
        return a - 2 * PI
    return a


def global_ld(tab, s, ey):
    """getGlobalPosition in long double on the row of lookup_row: (x, y, theta, row); NaNs and row -1 where the rule finds none."""
    i, w = lookup_row(tab, s)
    if i < 0:
        nan = LD(np.nan)
        return nan, nan, nan, -1
    T = tab.astype(LD)
    s, ey = LD(w), LD(ey)
    if tab[i, 5] == 0.0:
        xf, yf, xs, ys, psi = T[i, 0], T[i, 1], T[i - 1, 0], T[i - 1, 1], T[i, 2]
        dL, rL = T[i, 4], s - T[i, 3]
        x = (1 - rL / dL) * xs + rL / dL * xf + ey * np.cos(psi + PI / 2)
        y = (1 - rL / dL) * ys + rL / dL * yf + ey * np.sin(psi + PI / 2)
        return x, y, psi, i
    r = 1 / T[i, 5]; ang = T[i - 1, 2]
    d = 1 if r >= 0 else -1
    cx = T[i - 1, 0] + np.abs(r) * np.cos(ang + d * PI / 2)
    cy = T[i - 1, 1] + np.abs(r) * np.sin(ang + d * PI / 2)
    span = (s - T[i, 3]) / (PI * np.abs(r)) * PI
    an = _wrap_ld(d * PI / 2 + ang)
    a0 = -(PI - np.abs(an)) * _sgn(an)
    return cx + (np.abs(r) - d * ey) * np.cos(a0 + d * span), cy + (np.abs(r) - d * ey) * np.sin(a0 + d * span), ang + d * span, i


def _angle(p1x, p1y, ox, oy, p2x, p2y):
    v1x, v1y, v2x, v2y = p1x - ox, p1y - oy, p2x - ox, p2y - oy
    return np.arctan2(v1x * v2y - v1y * v2x, v1x * v2x + v1y * v2y)


class _Run(object):
    """One evaluation: the decisions taken, forced where `force` says so."""

    def __init__(self, force, strict_width=False):
        self.force, self.under, self.min_margin, self.strict_width = force, [], np.inf, strict_width

    def dec(self, key, margin, natural):
        m = abs(float(margin))
        self.min_margin = min(self.min_margin, m)
        if m < TAU:
            self.under.append(key)
            if key in self.force:
                return self.force[key]
        return bool(natural)


def locate(tab, hw, slack, x, y, force=None, strict_width=False):
    """The position part of getLocalPosition in long double.  Returns (row, branch, s, ey, base, run): the accepting row (-1: off the
    track), its branch ("start", "end", "in"), s and ey (long double) and the heading `base` that epsi is unwrapped against.
    strict_width is the mutant of the host test: `<` for `<=` in the width test."""
    run = _Run(force or {}, strict_width)
    T = tab.astype(LD)
    x, y = LD(x), LD(y)
    wlim = LD(np.float64(hw) + np.float64(slack))

    def width(i, ey):
        m = wlim - np.abs(ey)
        return run.dec(("w", i), m, m > 0 if strict_width else m >= 0)

    for i in range(tab.shape[0]):
        xf, yf, xs, ys = T[i, 0], T[i, 1], T[i - 1, 0], T[i - 1, 1]
        if tab[i, 5] == 0.0:
            base = T[i - 1, 2]
            if xs == x and ys == y:
                return i, "start", T[i, 3], LD(0), base, run
            if xf == x and yf == y:
                return i, "end", T[i, 3] + T[i, 4], LD(0), base, run
            a1 = _angle(x, y, xs, ys, xf, yf)
            if not run.dec(("a1", i), PI / 2 - np.abs(a1), np.abs(a1) <= PI / 2):
                continue
            a2 = _angle(x, y, xf, yf, xs, ys)
            if not run.dec(("a2", i), PI / 2 - np.abs(a2), np.abs(a2) <= PI / 2):
                continue
            n1 = np.sqrt((x - xs) * (x - xs) + (y - ys) * (y - ys))
            a = _angle(xf, yf, xs, ys, x, y)
            s, ey = n1 * np.cos(a) + T[i, 3], n1 * np.sin(a)
            if width(i, ey):
                return i, "in", s, ey, base, run
        else:
            r = 1 / T[i, 5]
            d = 1 if r >= 0 else -1
            ang = T[i - 1, 2]
            cx = xs + np.abs(r) * np.cos(ang + d * PI / 2)
            cy = ys + np.abs(r) * np.sin(ang + d * PI / 2)
            if xs == x and ys == y:
                return i, "start", T[i, 3], LD(0), ang, run
            if xf == x and yf == y:
                return i, "end", T[i, 3] + T[i, 4], LD(0), T[i, 2], run
            arc1 = T[i, 4] * T[i, 5]
            arc2 = _angle(xs, ys, cx, cy, x, y)
            true_pi = LD(np.pi) + LD(1.2246467991473532e-16)          # pi itself, to long double: arctan2's own edge
            if not run.dec(("sg", i), min(np.abs(arc2), true_pi - np.abs(arc2)), np.sign(arc1) == np.sign(arc2)):
                continue
            if not run.dec(("ar", i), np.abs(arc1) - np.abs(arc2), np.abs(arc1) >= np.abs(arc2)):
                continue
            s = np.abs(arc2) * np.abs(r) + T[i, 3]
            ey = -d * (np.sqrt((x - cx) * (x - cx) + (y - cy) * (y - cy)) - np.abs(r))
            if width(i, ey):
                return i, "in", s, ey, ang + arc2, run
    return -1, "off", LD(10000), LD(10000), LD(0), run


def unwrap_ld(base, psi, force=None):
    """numpy.unwrap([base, psi])[1] - base in long double: (epsi, margin, turns).  The decision is how many whole turns are taken off
    psi; margin is the distance of psi - base from the nearest odd multiple of pi, `force` takes the other side of that half turn."""
    dd = LD(psi) - LD(base)
    k = np.floor((dd + PI) / (2 * PI))                     # dd - 2 pi k in [-pi, pi)
    red = dd - 2 * PI * k
    if red == -PI and dd > 0:                              # numpy keeps +pi for a positive step
        k = k - 1
    if np.abs(dd) < PI:
        k = LD(0)
    q = np.abs(dd) / PI
    odd = 2 * np.floor(q / 2) + 1
    margin = float(np.abs(np.abs(dd) - odd * PI))
    if force:                                              # the other side of the half turn
        k = k - 1 if dd - 2 * PI * k < 0 else k + 1
    return (LD(psi) - 2 * PI * k) - LD(base), margin, int(k)


class Expect(object):
    """What a local case may return: `rows` [v, 5] = (s, ey, epsi, inside, row) of every variant (one when decided)."""
    __slots__ = ("decided", "rows", "branch", "min_margin")

    def __init__(self, decided, rows, branch, min_margin):
        self.decided, self.rows, self.branch, self.min_margin = decided, rows, branch, min_margin


def _variants(tab, hw, slack, x, y, strict_width=False):
    """Every position outcome: [(row, branch, s, ey, base)], decided flag, smallest margin."""
    out, stack, first = [], [{}], None
    while stack:
        f = stack.pop()
        row, br, s, ey, base, run = locate(tab, hw, slack, x, y, f, strict_width)
        if first is None:
            first = run
        todo = [k for k in run.under if k not in f]
        if todo:
            for outcome in (True, False):
                g = dict(f); g[todo[0]] = outcome
                stack.append(g)
            if len(stack) + len(out) > 64:
                raise RuntimeError("too many forced variants at (%r, %r)" % (x, y))
            continue
        out.append((row, br, s, ey, base))
    return out, not first.under, first.min_margin


def expect_local(tab, hw, slack, x, y, psis, strict_width=False):
    """[Expect] for the headings psis at one point: positions once, the unwrap per heading."""
    pos, decided, mm = _variants(tab, hw, slack, x, y, strict_width)
    res = []
    for psi in psis:
        rows, dec, m = [], decided, mm
        for row, br, s, ey, base in pos:
            if row < 0:
                rows.append((10000.0, 10000.0, 10000.0, 0.0, -1.0))
                continue
            e, mg, _ = unwrap_ld(base, psi)
            m = min(m, mg)
            rows.append((float(s), float(ey), float(e), 1.0, float(row)))
            if mg < TAU:
                dec = False
                rows.append((float(s), float(ey), float(unwrap_ld(base, psi, True)[0]), 1.0, float(row)))
        uniq = sorted(set(rows))
        res.append(Expect(dec, np.array(uniq), pos[0][1], m))
    return res


def local_ld(tab, hw, slack, x, y, psi, strict_width=False):
    """The unforced restatement of getLocalPosition: (s, ey, epsi, inside) as floats."""
    row, br, s, ey, base, _ = locate(tab, hw, slack, x, y, None, strict_width)
    if row < 0:
        return 10000.0, 10000.0, 10000.0, 0
    return float(s), float(ey), float(unwrap_ld(base, psi)[0]), 1


# ---- the grid's points -------------------------------------------------------------------------------------------------------
KIND_GRID, KIND_END, KIND_WIDTH = 0, 1, 2


def global_points(m):
    """(s, ey) [n, 2] and the s grid's seam, DS and lap indices repeated per ey."""
    tab = np.asarray(m.PointAndTangent, float)
    s, j, d, lap = s_grid(tab)
    ey = ey_grid(m)
    sey = np.column_stack([np.repeat(s, ey.size), np.tile(ey, s.size)])
    return sey, np.repeat(j, ey.size), np.repeat(d, ey.size), np.repeat(lap, ey.size)


def local_points(m):
    """The local cases of one track, cases of the same (x, y) adjacent: dict of pts [n, 3] = (x, y, psi), pos [n] (index of the
    (x, y)), kind, seam, ds, lap, iey, idpsi [n] (int32; -1 where it does not apply)."""
    tab = np.asarray(m.PointAndTangent, float)
    sey, j, d, lap = global_points(m)
    rng = np.random.default_rng(HEADING_SEED)
    ney = ey_grid(m).size
    rec = []

    def add(x, y, th, heads, kind, jj, dd, ll, ie):
        p = rec[-1][0] + 1 if rec else 0
        for h in heads:
            rec.append((p, x, y, th + DPSI[h], kind, jj, dd, ll, ie, h))

    for n in range(sey.shape[0]):
        if (j[n] < 0 and not np.isfinite(sey[n, 0])) or (lap[n] > 0 and d[n] < 3):
            continue
        try:
            x, y, th = PR.get_global_position(tab, sey[n, 0], sey[n, 1])
        except ValueError:
            continue
        second = int(rng.integers(1, N_PLAIN))                          # drawn for every point, so the stream does not depend on the branch
        wide = j[n] >= 0 and d[n] >= 3
        if wide and lap[n] == 0:
            heads = list(range(N_PLAIN))
            if j[n] in (1, 2, 3) and DS[d[n]] == 1e-3 and n % ney == 0:
                heads += list(range(N_PLAIN, len(DPSI)))
        elif wide:
            heads = [0, second]
        else:
            heads = [0]
        add(float(x), float(y), float(th), heads, KIND_GRID, j[n], d[n], lap[n], n % ney)
    w = float(m.halfWidth) + float(m.slack)
    for i in range(tab.shape[0]):
        add(float(tab[i, 0]), float(tab[i, 1]), float(tab[i, 2]), range(len(DPSI)), KIND_END, i, -1, 0, -1)
        if tab[i, 5] == 0.0 and tab[i, 4] > 1e-3:
            for sg in (1.0, -1.0):
                x, y, th = PR.get_global_position(tab, tab[i, 3] + tab[i, 4] / 2, sg * w)
                add(float(x), float(y), float(th), [0], KIND_WIDTH, i, -1, 0, -1)
    a = np.array(rec, float)
    out = dict(pts=np.ascontiguousarray(a[:, 1:4]), pos=a[:, 0].astype(np.int32))
    for c, k in enumerate(("kind", "seam", "ds", "lap", "iey", "idpsi")):
        out[k] = a[:, 4 + c].astype(np.int32)
    return out


def expectations(m, loc):
    """[Expect] for the local cases `loc` of local_points(m)."""
    tab = np.asarray(m.PointAndTangent, float)
    pts, pos = loc["pts"], loc["pos"]
    out, n = [], 0
    while n < pts.shape[0]:
        e = n
        while e < pts.shape[0] and pos[e] == pos[n]:
            e += 1
        out.extend(expect_local(tab, m.halfWidth, m.slack, pts[n, 0], pts[n, 1], pts[n:e, 2]))
        n = e
    return out


_CACHE = {}


def grid():
    """The whole grid, built once per process: a list, one dict per track, of map, tab, glob (sey, seam, ds, lap, row, wrapped),
    loc (local_points) and exp (expectations)."""
    if "grid" not in _CACHE:
        G = []
        for t, m in enumerate(tracks()):
            tab = np.asarray(m.PointAndTangent, float)
            sey, j, d, lap = global_points(m)
            rw = [lookup_row(tab, s) for s in sey[:, 0]]
            loc = local_points(m)
            G.append(dict(t=t, map=m, tab=tab, glob=dict(sey=sey, seam=j, ds=d, lap=lap, row=np.array([r[0] for r in rw], np.int32),
                                                          wrapped=np.array([r[1] for r in rw])),
                          loc=loc, exp=expectations(m, loc)))
        _CACHE["grid"] = G
    return _CACHE["grid"]


def check_local(got, exp, bounds=None):
    """Compare device rows got [n, 4] with the expectations: (bad case indices, worst deviation [3] of (s, ey, epsi) over the decided
    cases).  A decided case must have the inside flag and the sentinels exactly and every coordinate within its bound (LOCAL_BOUNDS);
    an undecided one must be within the bounds of one of its variants."""
    bounds = np.array(LOCAL_BOUNDS if bounds is None else bounds)
    bad, worst = [], np.zeros(3)
    for n, e in enumerate(exp):
        best = None
        for v in e.rows:
            if got[n, 3] != v[3]:
                continue
            if v[3] == 0:
                dev = np.zeros(3) if np.all(got[n, :3] == 10000) else np.full(3, np.inf)
            else:
                dev = np.abs(got[n, :3] - v[:3])
            if np.all(dev <= bounds) and (best is None or dev.max() < best.max()):
                best = dev
        if best is None:
            bad.append(n)
        elif e.decided:
            worst = np.maximum(worst, best)
    return bad, worst
