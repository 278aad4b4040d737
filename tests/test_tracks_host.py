"""CPU: per-vehicle tracks (include/lpvmpc.h, "Per-vehicle tracks") -- the exports of the built library, the track constructors of
track.py (from_segments, mirrored, scaled) against their construction, and the argument checks of track.pack_tracks, which
BatchedSolver.set_tracks runs before the library sees anything."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import _tracks as TK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ("oval", "L_shape", "3110", "Euge_Track")


def roundoff_bar(tab):
    """The round-off bar of a table against its construction: build_table forms every row from the row before it in at most 16
    rounded operations (two trigonometric calls, the centre, the end point, the arc length), each within one ulp of a word no larger
    than the table's largest; the errors add up along the rows."""
    return 16 * tab.shape[0] * np.finfo(float).eps * float(np.max(np.abs(tab)))


def test_library_exports_the_binding():
    import lpvmpc
    lib = C.CDLL(lpvmpc._ffi.LIB_PATH)
    for name in ("lpvmpc_set_tracks", "lpvmpc_tracks_read"):
        assert hasattr(lib, name), name
        assert name in lpvmpc._ffi.EXPORTS
    h = open(os.path.join(ROOT, "include", "lpvmpc.h")).read()
    assert re.search(r"#define\s+LPVMPC_MAX_TRACKS\s+64\b", h) and lpvmpc._ffi.MAX_TRACKS == 64
    assert "lpvmpc_set_tracks(lpvmpc_handle *h, int32_t T, const int32_t *track_rows" in h


def test_from_segments_rebuilds_the_shipped_tracks():
    from lpvmpc import track as T
    for shape in SHAPES:
        m = T.Map(shape, 0.2)
        c = T.Map.from_segments(T.TRACK_SPECS[shape][0], m.halfWidth, m.slack)
        assert np.array_equal(c.PointAndTangent, m.PointAndTangent) and c.TrackLength == m.TrackLength
        assert (c.halfWidth, c.slack) == (m.halfWidth, m.slack)
        # the segments read back from a table (a map without a segment list, such as the reference's own Map) rebuild it
        class Bare(object):
            PointAndTangent, halfWidth, slack = m.PointAndTangent, m.halfWidth, m.slack
        assert np.max(np.abs(T.scaled(Bare, 1.0).PointAndTangent - m.PointAndTangent)) <= 1e-14
    for bad in ([], [(0.0, 0)], [(-1.0, 0)], [(1.0, np.nan)], [(np.inf, 0)]):
        with pytest.raises(ValueError):
            T.Map.from_segments(bad, 0.3, 0.1)
    for hw, sl in ((-0.1, 0.1), (0.3, -0.1), (np.nan, 0.1), (0.3, np.inf)):
        with pytest.raises(ValueError):
            T.Map.from_segments([(1.0, 0)], hw, sl)


@pytest.mark.parametrize("shape", SHAPES)
def test_mirrored_reflects_y_and_psi(shape):
    """mirrored(m): x, cum_s and seg_len of every row are m's, y, psi and the curvature change sign; the closing row returns to the
    origin; mirrored(mirrored(m)) reproduces m.  psi is compared as an angle (modulo 2 pi).  Both differences are held at
    roundoff_bar (4e-13 .. 1e-12 on these tables); measured on the four shipped tracks: at most 4.4e-16 in any word of mirrored(m)
    against the reflection of m, and 0 in mirrored(mirrored(m)) against m."""
    from lpvmpc import track as T
    m = T.Map(shape, 0.2)
    r = T.mirrored(m)
    a, b = m.PointAndTangent, r.PointAndTangent
    assert a.shape == b.shape and (r.halfWidth, r.slack) == (m.halfWidth, m.slack)
    d = b - a * np.array([1.0, -1.0, -1.0, 1.0, 1.0, -1.0])
    d[:, 2] = (d[:, 2] + np.pi) % (2 * np.pi) - np.pi                 # psi is an angle: build_table wraps a heading of +-pi by round-off
    err = float(np.max(np.abs(d)))
    back = float(np.max(np.abs(T.mirrored(r).PointAndTangent - a)))
    print("%s: mirrored against the reflection %.2e, mirrored twice against the track %.2e" % (shape, err, back))
    assert err <= roundoff_bar(a) and back <= roundoff_bar(a)
    assert np.all(np.sign(b[:, 5]) == -np.sign(a[:, 5]))
    assert np.all(b[-1, :3] == 0.0) and b[-1, 5] == 0.0 and abs(r.TrackLength - m.TrackLength) <= roundoff_bar(a)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("k", (1.3, 0.5))
def test_scaled_multiplies_lengths_and_divides_curvature(shape, k):
    """scaled(m, k): x, y, cum_s and seg_len of every row are k times m's, psi is m's (as an
    angle: modulo 2 pi), the curvature m's divided by k; the closing row returns to the origin.  Held at roundoff_bar of the scaled
    table; measured: at most 1.1e-14 in any word (3110 x 1.3).  The closing gap of the oval is itself round-off, 6e-16, and is not
    scaled: it stays inside the bar."""
    from lpvmpc import track as T
    m = T.Map(shape, 0.2)
    r = T.scaled(m, k)
    a, b = m.PointAndTangent, r.PointAndTangent
    d = b - a * np.array([k, k, 1.0, k, k, 1.0 / k])
    d[:, 2] = (d[:, 2] + np.pi) % (2 * np.pi) - np.pi                 # psi is an angle: build_table wraps a heading of +-pi by round-off
    err = float(np.max(np.abs(d)))
    print("%s x %g: against the construction %.2e" % (shape, k, err))
    assert a.shape == b.shape and err <= roundoff_bar(b)
    assert np.all(b[-1, :3] == 0.0) and b[-1, 5] == 0.0 and abs(r.TrackLength - k * m.TrackLength) <= roundoff_bar(b)
    assert (r.halfWidth, r.slack) == (m.halfWidth, m.slack)
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            T.scaled(m, bad)


def test_palette_of_the_gpu_tests():
    """Six closed tracks of different row counts and lengths that the library's own rules accept (every segment length > 0)."""
    maps = TK.palette()
    assert [m.PointAndTangent.shape[0] for m in maps] == [6, 7, 12, 14, 7, 6]
    assert len(set(np.round(TK.lengths(maps), 6))) == 5               # the mirrored L shape has the L shape's length
    for m in maps:
        assert np.all(m.PointAndTangent[:, 4] > 0) and np.all(np.isfinite(m.PointAndTangent))
    assert TK.cycle(8).tolist() == [0, 1, 2, 3, 4, 5, 0, 1]


def test_pack_tracks_layout_and_checks():
    from lpvmpc.track import pack_tracks
    maps = TK.palette()
    of = TK.cycle(9)
    rows, tab, hw, sl, o = pack_tracks(maps, of)
    assert rows.dtype == np.int32 and o.dtype == np.int32 and tab.shape == (6, 16, 6) and tab.flags["C_CONTIGUOUS"]
    for t, m in enumerate(maps):
        n = m.PointAndTangent.shape[0]
        assert rows[t] == n and np.array_equal(tab[t, :n], m.PointAndTangent) and np.all(tab[t, n:] == 0.0)
        assert hw[t] == m.halfWidth and sl[t] == m.slack
    assert np.array_equal(o, of)
    assert pack_tracks(maps[0], [0, 0])[0].tolist() == [6]              # a single map is a palette of one

    class Bad(object):
        def __init__(self, m, **kw):
            self.PointAndTangent, self.halfWidth, self.slack = m.PointAndTangent.copy(), m.halfWidth, m.slack
            for k, v in kw.items():
                setattr(self, k, v)

    nan = Bad(maps[1]); nan.PointAndTangent[2, 0] = np.nan
    zero = Bad(maps[1]); zero.PointAndTangent[3, 4] = 0.0
    for palette, track_of in (([], [0]), (maps * 11, [0]), ([Bad(maps[0], PointAndTangent=np.zeros((17, 6)))], [0]),
                              ([Bad(maps[0], PointAndTangent=np.ones((1, 6)))], [0]), ([Bad(maps[0], PointAndTangent=np.ones((4, 5)))], [0]),
                              ([nan], [0]), ([zero], [0]), ([Bad(maps[0], halfWidth=-0.1)], [0]), ([Bad(maps[0], slack=np.nan)], [0]),
                              (maps, [0, 6]), (maps, [-1]), (maps, []), (maps, [[0, 1]]), (maps, [0.0, 1.0])):
        with pytest.raises(ValueError):
            pack_tracks(palette, track_of)


def test_fleet_tracks_checks_of_race_fleet():
    """track.fleet_tracks, which RaceFleet(track_map=..., track_of=...) runs before it creates an engine: one map (or a sequence of
    one) without track_of keeps the unbound path; a palette needs track_of with one entry per vehicle inside the palette."""
    from lpvmpc.track import fleet_tracks
    maps = TK.palette()
    assert fleet_tracks(maps[0], None, 5) == ([maps[0]], None)
    assert fleet_tracks([maps[1]], None, 5) == ([maps[1]], None)
    m, of = fleet_tracks(maps, TK.cycle(12), 12)
    assert m == maps and of.dtype == np.int32 and np.array_equal(of, TK.cycle(12))
    m, of = fleet_tracks(maps[2], np.zeros(3, int), 3)                  # a single map with track_of: a palette of one, bound
    assert m == [maps[2]] and np.array_equal(of, [0, 0, 0])
    for track_map, track_of, B in (([], None, 3), (maps, None, 12), (maps, TK.cycle(11), 12), (maps, [0, 6, 1], 3), (maps, [0.0, 1.0], 2),
                                   (maps * 11, TK.cycle(12), 12)):
        with pytest.raises(ValueError):
            fleet_tracks(track_map, track_of, B)
    import inspect
    import lpvmpc
    assert "track_of" in inspect.signature(lpvmpc.RaceFleet.__init__).parameters and hasattr(lpvmpc.RaceFleet, "tracks")


def test_pinned_race_event_ticks_are_the_host_replays():
    """The event ticks written into the mixed race test (tests/_tracks.py RACE_EVENT_TICKS) are what the host replay gives for
    its starts: after the 9 seed ticks, at least two different ticks, three vehicles on each of the four tracks."""
    maps, of = TK.race_palette(), TK.cycle(TK.RACE_B, 4)
    ev = TK.race_event_ticks(maps, of, TK.race_starts(maps, of))
    assert ev.tolist() == list(TK.RACE_EVENT_TICKS)
    assert ev.min() >= 9 and len(set(ev.tolist())) >= 2 and np.bincount(of).tolist() == [3, 3, 3, 3]
    assert len(set(np.round(TK.lengths(maps), 3))) == 4
