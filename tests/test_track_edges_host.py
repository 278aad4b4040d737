"""The edge grid of the track geometry on the host (tests/_track_edges.py): the float64 oracle against the reference's recorded
answers (tests/golden/track_edges/), the long double restatement against the oracle and against the reference, the mutant that
shows the restatement's width test is pinned, and the caps that keep the grid honest.  No GPU."""
import os

import numpy as np
import pytest

from oracle import lpv_ref as L
from oracle import plant_ref as PR
from tests import _track_edges as E

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "track_edges", "track_edges.npz")
TOL = 1e-12              # tests/test_oracle_plant.py


@pytest.fixture(scope="module")
def fx():
    return np.load(FIX)


@pytest.fixture(scope="module")
def grid():
    return E.grid()


@pytest.fixture(scope="module")
def oracle_local(grid):
    """oracle/plant_ref.py's get_local_position on every local case, once."""
    return [np.array([PR.get_local_position(g["tab"], g["map"].halfWidth, g["map"].slack, *p) for p in g["loc"]["pts"]], float) for g in grid]


def oracle_global(tab, s, ey):
    """(x, y, theta) or None where the oracle raises.  s = +inf is not passed on: like the reference it would subtract L for ever."""
    try:
        return PR.get_global_position(tab, s, ey)
    except ValueError:
        return None


def test_fixture_is_the_grid(fx, grid):
    for g in grid[:4]:
        sh = g["map"].shape
        assert np.array_equal(fx[sh + "_table"], g["tab"])
        sey = g["glob"]["sey"]
        assert np.array_equal(fx[sh + "_g_sey"], sey[~np.isposinf(sey[:, 0])], equal_nan=True)
        assert np.array_equal(np.column_stack([fx[sh + "_l_x"], fx[sh + "_l_y"], fx[sh + "_l_psi"]]), g["loc"]["pts"])


def test_oracle_against_the_fixture(fx, grid, oracle_local):
    """oracle/plant_ref.py and oracle.lpv_ref.curvature on the reference's points: raise flags and inside flags exactly, the curvature
    exactly, the coordinates to 1e-12.  The rules of tests/_track_edges.py find a row exactly where the reference answers, but for
    the one abscissa beyond kMaxWrapLaps laps, which the library documents as NaN."""
    for t, g in enumerate(grid[:4]):
        sh, tab = g["map"].shape, g["tab"]
        top = E.MAX_WRAP_LAPS * E.lap_length(tab)
        worst = 0.0
        for n, (s, ey) in enumerate(fx[sh + "_g_sey"]):
            o = oracle_global(tab, s, ey)
            assert (o is None) == bool(fx[sh + "_g_raised"][n]), (sh, s, ey)
            assert (E.lookup_row(tab, s)[0] < 0) == (o is None or s > top), (sh, s)
            if o is not None:
                worst = max(worst, float(np.max(np.abs(np.array(o, float) - fx[sh + "_g_out"][n]))))
        for n, s in enumerate(fx[sh + "_c_s"]):
            try:
                c = L.curvature(s, tab)
            except ValueError:
                c = None
            assert (c is None) == bool(fx[sh + "_c_raised"][n]), (sh, s)
            if c is not None:
                assert c == fx[sh + "_c_out"][n], (sh, s)
                if s <= top:
                    assert E.curvature_rule(tab, s) == c, (sh, s)
        ref = np.column_stack([fx[sh + "_l_s"], fx[sh + "_l_ey"], fx[sh + "_l_epsi"], fx[sh + "_l_inside"]])
        assert not fx[sh + "_l_raised"].any()
        assert np.array_equal(oracle_local[t][:, 3], ref[:, 3]), sh
        wl = float(np.max(np.abs(oracle_local[t] - ref)))
        print("%s: oracle - reference, global %.2e, local %.2e" % (sh, worst, wl))
        assert worst <= TOL and wl <= TOL


def test_restatement_against_the_oracle(grid, oracle_local):
    """On every decided case the long double restatement and the float64 oracle agree: flags exactly, coordinates within the
    recorded ORACLE_DEV_* (the figures the GPU bounds are derived from), separately for local (s, ey), local epsi and global."""
    wl = we = wg = 0.0
    for t, g in enumerate(grid):
        tab = g["tab"]
        for n, e in enumerate(g["exp"]):
            if e.decided:
                o, v = oracle_local[t][n], e.rows[0]
                assert o[3] == v[3], (g["map"].shape, n, o, v)
                wl = max(wl, float(np.max(np.abs(o[:2] - v[:2]))))
                we = max(we, float(abs(o[2] - v[2])))
        for (s, ey), row in zip(g["glob"]["sey"], g["glob"]["row"]):
            if row >= 0:
                o = oracle_global(tab, s, ey)
                assert o is not None
                x, y, th, r2 = E.global_ld(tab, s, ey)
                assert r2 == row
                wg = max(wg, float(max(abs(x - o[0]), abs(y - o[1]), abs(th - o[2]))))
            elif np.isfinite(s) and s <= E.MAX_WRAP_LAPS * E.lap_length(tab):
                assert oracle_global(tab, s, ey) is None
    print("worst |oracle - long double| on the decided grid: local s, ey %.3e, local epsi %.3e, global %.3e; GPU bounds %.1e %.1e %.1e"
          % (wl, we, wg, E.GPU_BOUND_LOCAL, E.GPU_BOUND_EPSI, E.GPU_BOUND_GLOBAL))
    assert wl <= E.ORACLE_DEV_LOCAL and we <= E.ORACLE_DEV_EPSI and wg <= E.ORACLE_DEV_GLOBAL
    for dev, bound in ((E.ORACLE_DEV_LOCAL, E.GPU_BOUND_LOCAL), (E.ORACLE_DEV_EPSI, E.GPU_BOUND_EPSI), (E.ORACLE_DEV_GLOBAL, E.GPU_BOUND_GLOBAL)):
        assert bound <= 1e-11 and bound == min(100 * dev, 1e-11)
    # a recorded figure may round the measured one up, by no more than a tenth
    assert wl >= 0.9 * E.ORACLE_DEV_LOCAL and we >= 0.9 * E.ORACLE_DEV_EPSI and wg >= 0.9 * E.ORACLE_DEV_GLOBAL


def test_restatement_against_the_reference_and_the_mutant(fx, grid):
    """On the fixture's decided points the restatement equals the reference's answers.  Its mutant with `<` for `<=` in the width
    test can differ from it only where |ey| equals hw + slack to the last bit of the long double: a width margin of 0, so by this
    file's own definition an UNDECIDED case, which round-off decides.  No decided case can tell the two apart, and this test does not
    claim one does.  What it shows is narrower: on the grid's points placed exactly hw + slack off a straight (KIND_WIDTH), the
    unforced restatement takes the side the reference took on at least one point where the mutant takes the other (seven of the
    points, all of which the reference accepts)."""
    caught = 0
    for g in grid[:4]:
        sh, tab, m = g["map"].shape, g["tab"], g["map"]
        ref = np.column_stack([fx[sh + "_l_s"], fx[sh + "_l_ey"], fx[sh + "_l_epsi"], fx[sh + "_l_inside"]])
        for n, e in enumerate(g["exp"]):
            if e.decided:
                assert ref[n, 3] == e.rows[0, 3] and np.max(np.abs(ref[n, :3] - e.rows[0, :3])) <= TOL, (sh, n)
        for n in np.nonzero(g["loc"]["kind"] == E.KIND_WIDTH)[0]:
            p = g["loc"]["pts"][n]
            good, bad = E.local_ld(tab, m.halfWidth, m.slack, *p), E.local_ld(tab, m.halfWidth, m.slack, *p, strict_width=True)
            if good[3] == ref[n, 3] and bad[3] != ref[n, 3]:
                caught += 1
    print("the width mutant is caught on %d grid points" % caught)
    assert caught >= 1


def test_caps(grid):
    """Conditions on the grid, not measurements."""
    n_all = n_und = 0
    kinds = set()
    for g in grid:
        tab, loc, exp = g["tab"], g["loc"], g["exp"]
        sh = g["map"].shape
        n_all += len(exp); n_und += sum(not e.decided for e in exp)
        assert max(e.rows.shape[0] for e in exp) <= E.MAX_VARIANTS, sh
        dec_in = np.array([e.decided and e.rows[0, 3] == 1 for e in exp])
        nseam = tab.shape[0] + 1
        for j in range(nseam):
            # the lap end and the start line are one place: before it is L - 1e-9, after it 0 + 1e-9
            for d, jj in ((3, nseam - 1 if j == 0 else j), (4, 0 if j == nseam - 1 else j)):
                assert np.any(dec_in & (loc["seam"] == jj) & (loc["ds"] == d) & (loc["kind"] == E.KIND_GRID) & (loc["lap"] == 0)), (sh, j, d)
        taken = {(int(e.rows[0, 4]), e.branch) for e in exp if e.decided and e.rows[0, 3] == 1}
        for i in range(tab.shape[0]):
            # every row; a closing row that is 6e-16 m long or points backwards (the first straight takes its points) has no inside
            # of its own and is entered by the lookups of the global grid alone, which are decided by construction
            # (a 6e-16 m row is empty in float64, start + len == start: nothing can enter it, and s = L finds no row at all)
            last = i == tab.shape[0] - 1
            assert (i, "in") in taken or (last and (np.any(g["glob"]["row"] == i) or tab[i, 3] + tab[i, 4] == tab[i, 3])), (sh, i)
        kinds |= {(float(np.sign(tab[i, 5])), b) for i, b in taken}
        assert g["glob"]["row"].shape[0] == g["glob"]["sey"].shape[0]              # every lookup has its rule: decided by construction
    # both kinds of segment, both arc directions, every norm == 0 branch.  An arc's start point is the end point of the row before
    # it, which takes it first: only a track whose first row is an arc (Euge_Track, a left arc) reaches that branch
    assert {(k, b) for k in (0.0, 1.0, -1.0) for b in ("in", "end")} | {(0.0, "start"), (1.0, "start")} <= kinds, kinds
    print("local cases %d, undecided %d (%.2f %%)" % (n_all, n_und, 100.0 * n_und / n_all))
    assert n_und <= 0.05 * n_all


def test_long_double_against_50_digits(grid):
    """The restatement's arithmetic against the same statements at 50 digits, on a fixed sample of 200 decided inside-track points."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    pi64 = mp.mpf(float(np.pi))
    ang = lambda ax, ay, ox, oy, bx, by: mp.atan2((ax - ox) * (by - oy) - (ay - oy) * (bx - ox), (ax - ox) * (bx - ox) + (ay - oy) * (by - oy))
    cases = [(g, n) for g in grid for n, e in enumerate(g["exp"]) if e.decided and e.rows[0, 3] == 1 and e.branch == "in"]
    worst = 0.0
    for g, n in cases[::max(1, len(cases) // 200)][:200]:
        T, e = g["tab"], g["exp"][n]
        i = int(e.rows[0, 4])
        x, y, psi = [mp.mpf(float(v)) for v in g["loc"]["pts"][n]]
        xf, yf, xs, ys = [mp.mpf(float(v)) for v in (T[i, 0], T[i, 1], T[i - 1, 0], T[i - 1, 1])]
        if T[i, 5] == 0.0:
            n1, a = mp.sqrt((x - xs) ** 2 + (y - ys) ** 2), ang(xf, yf, xs, ys, x, y)
            s, ey, base = n1 * mp.cos(a) + mp.mpf(float(T[i, 3])), n1 * mp.sin(a), mp.mpf(float(T[i - 1, 2]))
        else:
            r = 1 / mp.mpf(float(T[i, 5])); d = 1 if r >= 0 else -1; a0 = mp.mpf(float(T[i - 1, 2]))
            cx, cy = xs + abs(r) * mp.cos(a0 + d * pi64 / 2), ys + abs(r) * mp.sin(a0 + d * pi64 / 2)
            arc2 = ang(xs, ys, cx, cy, x, y)
            s, ey, base = abs(arc2) * abs(r) + mp.mpf(float(T[i, 3])), -d * (mp.sqrt((x - cx) ** 2 + (y - cy) ** 2) - abs(r)), a0 + arc2
        k = E.unwrap_ld(E.LD(float(base)), float(psi))[2]
        epsi = psi - 2 * pi64 * k - base
        worst = max(worst, float(abs(s - mp.mpf(float(e.rows[0, 0])))), float(abs(ey - mp.mpf(float(e.rows[0, 1])))),
                    float(abs(epsi - mp.mpf(float(e.rows[0, 2])))))
    print("long double against 50 digits, 200 decided points: %.3e" % worst)
    assert worst <= 2e-15              # the expectation is kept as float64: half an ulp at 16 .. 32 m is 1.8e-15
