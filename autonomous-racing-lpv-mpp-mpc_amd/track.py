"""Track table for callers without the reference's ROS environment.

Mirror of ``Map.__init__`` (reference Utilities/trackInitialization.py:13-202): a track is a list of
(length, signed radius) segments turned into rows ``[x, y, psi, cum_s, seg_len, curvature]``
(``PointAndTangent``).  Only the table feeds the solve path (curvature lookup on the device,
csrc/lpvmpc_device.hpp ``track_curvature`` == Utilities/utilities.py:31-50); the coordinate
transforms (getGlobalPosition / getLocalPosition) are caller-side and out of this package's scope.

Any object exposing ``.PointAndTangent`` and ``.halfWidth`` -- e.g. the reference's own ``Map`` -- can be
passed to the drop-in classes instead.
"""
from __future__ import annotations

import math

import numpy as np

_PI = np.pi

TRACK_SPECS = {
    # shape: (segments as (length, radius; 0 = straight), fixed halfWidth or None, slack)   TRACK:28-81
    "oval": ([(1.0, 0), (4.5, 4.5 / _PI), (2.0, 0), (4.5, 4.5 / _PI), (1.0, 0)], None, 0.15),
    "L_shape": ([(1.0, 0), (4.5, 4.5 / _PI), (4.5 / 2, -4.5 / _PI), (4.5, 4.5 / _PI), (4.5 / _PI * 2, 0),
                 (4.5 / 2, 4.5 / _PI)], None, 0.45),
    "3110": ([(60 * 0.03, 0), (80 * 0.03, 80 * 0.03 * 2 / _PI), (20 * 0.03, 0), (80 * 0.03, 80 * 0.03 * 2 / _PI),
              (40 * 0.03, -40 * 0.03 * 10 / _PI), (60 * 0.03, 60 * 0.03 * 5 / _PI),
              (40 * 0.03, -40 * 0.03 * 10 / _PI), (80 * 0.03, 80 * 0.03 * 2 / _PI), (20 * 0.03, 0),
              (80 * 0.03, 80 * 0.03 * 2 / _PI), (80 * 0.03, 0)], 0.6, 0.15),
    "Euge_Track": ([(30 * 0.03, 30 * 0.03 * 2 / _PI), (20 * 0.03, 0), (30 * 0.03, -30 * 0.03 * 2 / _PI),
                    (30 * 0.03, 30 * 0.03 * 2 / _PI), (30 * 0.03, 30 * 0.03 * 2 / _PI), (130 * 0.03, 0),
                    (30 * 0.03, 30 * 0.03 * 2 / _PI), (10 * 0.03, 0), (30 * 0.03, 30 * 0.03 * 2 / _PI),
                    (55 * 0.03, 0), (30 * 0.03, -30 * 0.03 * 2 / _PI), (10 * 0.03, 0),
                    (30 * 0.03, 30 * 0.03 * 2 / _PI)], 0.4, 0.15),
}


def _wrap_pi(a):
    if a < -math.pi:
        return a + 2 * math.pi
    if a > math.pi:
        return a - 2 * math.pi
    return a


def build_table(segments):
    """Rows [x y psi cum_s len kappa] for each segment plus the closing row back to the origin."""
    n = len(segments)
    tab = np.zeros((n + 1, 6))
    px = py = heading = 0.0
    s_acc = 0.0
    for i, (length, radius) in enumerate(segments):
        if i > 0:
            px, py, heading = tab[i - 1, 0], tab[i - 1, 1], tab[i - 1, 2]
            s_acc = tab[i - 1, 3] + tab[i - 1, 4]
        if radius == 0:
            tab[i] = (px + length * np.cos(heading), py + length * np.sin(heading), heading, s_acc, length, 0.0)
            continue
        turn = 1 if radius >= 0 else -1
        rad = np.abs(radius)
        cx = px + rad * np.cos(heading + turn * _PI / 2)
        cy = py + rad * np.sin(heading + turn * _PI / 2)
        sweep = length / rad
        normal = _wrap_pi(turn * _PI / 2 + heading)
        start = -(_PI - np.abs(normal)) * (1 if normal >= 0 else -1)
        tab[i] = (cx + rad * np.cos(start + turn * sweep), cy + rad * np.sin(start + turn * sweep),
                  _wrap_pi(heading + sweep * np.sign(radius)), s_acc, length, 1 / radius)
    gap = np.sqrt((0 - tab[-2, 0]) ** 2 + (0 - tab[-2, 1]) ** 2)
    tab[-1] = (0.0, 0.0, 0.0, tab[-2, 3] + tab[-2, 4], gap, 0.0)
    return tab


class Map:
    """``Map(shape, halfWidth_param)``: ``.PointAndTangent``, ``.TrackLength``, ``.halfWidth``, ``.slack``.

    ``halfWidth_param`` plays the role of the ROS parameter /TrajectoryPlanner/halfWidth (the reference
    adds 0.1 to it, TRACK:20)."""

    def __init__(self, shape="oval", halfWidth_param=0.2):
        if shape not in TRACK_SPECS:
            raise ValueError("unknown track shape %r (have %s)" % (shape, sorted(TRACK_SPECS)))
        segments, fixed_hw, slack = TRACK_SPECS[shape]
        self.shape = shape
        self.segments = [(float(l), float(r)) for l, r in segments]
        self.slack = slack
        self.halfWidth = fixed_hw if fixed_hw is not None else halfWidth_param + 0.1
        self.PointAndTangent = build_table(segments)
        self.TrackLength = self.PointAndTangent[-1, 3] + self.PointAndTangent[-1, 4]
        self._eng = None

    @classmethod
    def from_segments(cls, segments, halfWidth, slack, shape="custom"):
        """A closed track from (length, signed radius; 0 = straight) segments with the given half width and slack: the table of
        ``build_table``, closing row included."""
        segments = [(float(l), float(r)) for l, r in segments]
        if not segments or any(not (l > 0) or not math.isfinite(l) or not math.isfinite(r) for l, r in segments):
            raise ValueError("segments must be a non-empty sequence of (length > 0, finite radius)")
        if not (math.isfinite(halfWidth) and halfWidth >= 0 and math.isfinite(slack) and slack >= 0):
            raise ValueError("halfWidth and slack must be finite and >= 0")
        m = cls.__new__(cls)
        m.shape, m.segments, m.slack, m.halfWidth = shape, segments, float(slack), float(halfWidth)
        m.PointAndTangent = build_table(segments)
        m.TrackLength = m.PointAndTangent[-1, 3] + m.PointAndTangent[-1, 4]
        m._eng = None
        return m

    # -- coordinate transforms of the reference's Map, evaluated by the device kernels (one point per call) ----------
    def _engine(self):
        if self._eng is None:
            from .api import BatchedSolver                  # raises LpvMpcError without a HIP device: no CPU fallback
            self._eng = BatchedSolver("controller", 8, 1.0 / 30.0, np.eye(6), np.eye(2), np.ones(2), track=self.PointAndTangent)
        return self._eng

    def getGlobalPosition(self, s, ey):
        """TRACK:205-262: (s, ey) -> (x, y, theta)."""
        x, y, th = self._engine().global_position(np.array([[float(s), float(ey)]]))[0]
        return float(x), float(y), float(th)

    def getLocalPosition(self, x, y, psi):
        """TRACK:283-383: (x, y, psi) -> (s, ey, epsi, insideTrack); 10000 sentinels when the point is off the track."""
        s, ey, epsi, inside = self._engine().local_position(np.array([[float(x), float(y), float(psi)]]), self.halfWidth, self.slack)[0]
        return float(s), float(ey), float(epsi), int(inside)


def _segments_of(m):
    """(length, signed radius) of every segment but the closing row, from the map's own list or from its table."""
    seg = getattr(m, "segments", None)
    if seg is not None:
        return list(seg)
    tab = np.asarray(m.PointAndTangent, dtype=np.float64)
    return [(float(r[4]), 0.0 if r[5] == 0 else float(1.0 / r[5])) for r in tab[:-1]]


def mirrored(m):
    """The track reflected in the x axis: every radius negated (left turns become right turns), the same lengths, half width and
    slack.  A closed track built with ``build_table``: y and psi of every row change sign, the curvature too."""
    return Map.from_segments([(l, -r if r != 0 else 0.0) for l, r in _segments_of(m)], m.halfWidth, m.slack,
                             shape="mirrored(%s)" % getattr(m, "shape", "map"))


def scaled(m, k):
    """The track k times as large: every length and radius times k, the same half width and slack.  A closed track built with
    ``build_table``: x, y, cum_s and seg_len of every row are multiplied by k, the curvature divided by it."""
    k = float(k)
    if not (k > 0 and math.isfinite(k)):
        raise ValueError("scale factor must be finite and > 0, got %r" % (k,))
    return Map.from_segments([(l * k, r * k) for l, r in _segments_of(m)], m.halfWidth, m.slack,
                             shape="scaled(%s, %g)" % (getattr(m, "shape", "map"), k))


from ._ffi import MAX_TRACK_ROWS, MAX_TRACKS          # LPVMPC_MAX_TRACK_ROWS, LPVMPC_MAX_TRACKS


def pack_tracks(maps, track_of):
    """The arrays of lpvmpc_set_tracks for a palette ``maps`` (objects with .PointAndTangent, .halfWidth, .slack) and the palette
    entry ``track_of`` [B] of each vehicle: (track_rows [T] int32, tables [T, 16, 6], half_width [T], slack [T], track_of [B]
    int32).  Raises ValueError for what the library would refuse."""
    maps = list(maps) if not hasattr(maps, "PointAndTangent") else [maps]
    T = len(maps)
    if not 1 <= T <= MAX_TRACKS:
        raise ValueError("a track palette has 1 .. %d entries, got %d" % (MAX_TRACKS, T))
    rows, tab = np.zeros(T, np.int32), np.zeros((T, MAX_TRACK_ROWS, 6))
    hw, sl = np.zeros(T), np.zeros(T)
    for t, m in enumerate(maps):
        pt = np.asarray(m.PointAndTangent, dtype=np.float64)
        if pt.ndim != 2 or pt.shape[1] != 6 or not 2 <= pt.shape[0] <= MAX_TRACK_ROWS:
            raise ValueError("track %d: PointAndTangent has shape %s, expected (2 .. %d, 6)" % (t, pt.shape, MAX_TRACK_ROWS))
        if not np.all(np.isfinite(pt)):
            raise ValueError("track %d: PointAndTangent has a non-finite word" % t)
        if not np.all(pt[:, 4] > 0):
            raise ValueError("track %d: segment lengths must be > 0 (row %d has %g)" % (t, int(np.argmin(pt[:, 4])), pt[:, 4].min()))
        hw[t], sl[t] = float(m.halfWidth), float(m.slack)
        if not (np.isfinite(hw[t]) and hw[t] >= 0 and np.isfinite(sl[t]) and sl[t] >= 0):
            raise ValueError("track %d: halfWidth and slack must be finite and >= 0" % t)
        rows[t] = pt.shape[0]
        tab[t, :pt.shape[0]] = pt
    of = np.asarray(track_of)
    if of.ndim != 1 or of.shape[0] < 1 or not np.issubdtype(of.dtype, np.integer):
        raise ValueError("track_of must be a non-empty 1-D integer array, one palette entry per vehicle")
    if of.min() < 0 or of.max() >= T:
        raise ValueError("track_of has entries outside 0 .. %d" % (T - 1))
    return rows, tab, hw, sl, np.ascontiguousarray(of, dtype=np.int32)


def fleet_tracks(track_map, track_of, B):
    """The tracks of a B-vehicle fleet: (maps, track_of).  One map (or a sequence of one) without track_of: ([map], None), the fleet
    runs on the handle's own track.  A sequence of maps with track_of [B]: the checked palette and indices (pack_tracks' rules)."""
    single = hasattr(track_map, "PointAndTangent")
    maps = [track_map] if single else list(track_map)
    if not maps:
        raise ValueError("track_map is an empty sequence")
    if track_of is None:
        if len(maps) != 1:
            raise ValueError("a palette of %d tracks needs track_of, the palette entry of each of the %d vehicles" % (len(maps), B))
        return maps, None
    of = pack_tracks(maps, track_of)[4]
    if of.shape[0] != B:
        raise ValueError("track_of has %d entries for %d vehicles" % (of.shape[0], B))
    return maps, of


def palette():
    """A six-entry palette for mixed fleets, benches and tests: the four shipped tracks, mirrored(L_shape) and scaled(oval, 1.3) --
    tables of 6, 7, 12, 14, 7 and 6 rows, lengths 13 .. 19.3 m, right and left turns, three half widths and two slacks."""
    return [Map("oval", 0.2), Map("L_shape", 0.2), Map("3110", 0.2), Map("Euge_Track", 0.2), mirrored(Map("L_shape", 0.2)),
            scaled(Map("oval", 0.2), 1.3)]


def cycle(B, T=6):
    """track_of [B] that cycles through a palette of T entries: vehicle b on entry b mod T."""
    return (np.arange(B) % T).astype(np.int32)
