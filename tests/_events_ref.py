"""The race event log (include/lpvmpc.h, "Race event log") in plain numpy: the rules of the header, one vehicle and one kind at a time,
with its own carry, and a model of the ring.  An event is the tuple (tick, kind, vehicle, other, a, b, v0, v1)."""
from __future__ import annotations

import numpy as np

LAP, FINISH, LOST, PASS, CONTACT_BEGIN, CONTACT_END, WALL_HIT, WALL_CLEAR = range(1, 9)
ALL_KINDS = 0x1FE
NAN = float("nan")
# channels of the heats' and the walls' output planes (LPVMPC_HEAT_*, LPVMPC_WALL_*)
H_PROGRESS, H_CLEARANCE = 0, 3
H_POSITION, H_NEAREST, H_CONTACT, H_CLASS = 0, 2, 3, 9
W_DEPTH, W_IMPULSE = 0, 1
W_HIT, W_SIDE, W_CORNER = 0, 1, 2


def key(ev):
    """The contract's order: (tick, vehicle, kind, other)."""
    return (ev[0], ev[2], ev[1], ev[3])


class EventsRef(object):
    """The log of B vehicles, stepped on the host.  ``kinds``: the mask (bit k selects kind k)."""

    def __init__(self, B, kinds=ALL_KINDS):
        self.B, self.kinds = int(B), int(kinds)
        self.seen = False                                       # the race's rows are stored
        self.phase = np.zeros(B, int); self.lap = np.zeros(B, int)
        self.seen_h = np.zeros(B, bool)                         # the heats' words of the vehicle are stored
        self.position = np.full(B, -1, int); self.cls = np.full(B, -1, int)
        self.contact = np.zeros(B, int); self.nearest = np.full(B, -1, int); self.contact_start = np.full(B, -1, int)
        self.min_clearance = np.zeros(B)
        self.seen_w = np.zeros(B, bool)
        self.hit = np.zeros(B, int); self.hit_start = np.full(B, -1, int); self.max_impulse = np.zeros(B)
        self.count = np.zeros(B, int); self.count_total = np.zeros(B, int)
        self.total = 0

    def step(self, t, phase, lap, lap_value, heats_planes=None, heat=None, walls_planes=None, heats_fresh=False, walls_fresh=False):
        """One tick: the race's rows after it, ``lap_value`` [B] the V0 of a LAP event, the heats' planes dict(f64 [5, B], i32 [10, B])
        with ``heat`` [B] (None: no heats), the walls' planes dict(f64 [4, B], i32 [6, B]) (None: no walls); ``*_fresh``: the source is
        an attachment the log has not seen (a replacement between two ticks).  Returns the tick's events in contract order."""
        B = self.B
        phase = np.asarray(phase, int); lap = np.asarray(lap, int); lap_value = np.asarray(lap_value, float)
        hf = hi = wf = wi = None
        if heats_planes is not None:
            hf, hi, heat = np.asarray(heats_planes["f64"], float), np.asarray(heats_planes["i32"], int), np.asarray(heat, int)
        if walls_planes is not None:
            wf, wi = np.asarray(walls_planes["f64"], float), np.asarray(walls_planes["i32"], int)
        out = []
        self.count[:] = 0

        def put(b, kind, other=-1, a=-1, bb=-1, v0=NAN, v1=NAN):
            if (self.kinds >> kind) & 1:
                out.append((int(t), kind, int(b), int(other), int(a), int(bb), float(v0), float(v1)))
                self.count[b] += 1

        for b in range(B):
            if self.seen:
                if lap[b] > self.lap[b]:
                    put(b, LAP, a=lap[b], bb=phase[b], v0=lap_value[b])
                if phase[b] == 2 and self.phase[b] != 2:
                    put(b, FINISH, a=lap[b])
                if phase[b] == 3 and self.phase[b] != 3:
                    put(b, LOST, a=lap[b])
            has_h = hf is not None and heat[b] >= 0
            if has_h:
                seen = self.seen_h[b] and not heats_fresh
                pos, cls = hi[H_POSITION, b], hi[H_CLASS, b]
                con, near, clear = int(hi[H_CONTACT, b] != 0), hi[H_NEAREST, b], hf[H_CLEARANCE, b]
                con0 = self.contact[b] if seen else 0
                if seen and self.cls[b] == 1 and cls == 1:
                    for j in np.nonzero(heat == heat[b])[0]:
                        if j != b and self.cls[j] == 1 and hi[H_CLASS, j] == 1 and self.position[b] > self.position[j] and pos < hi[H_POSITION, j]:
                            put(b, PASS, other=j, a=pos, bb=hi[H_POSITION, j], v0=np.float64(hf[H_PROGRESS, b]) - np.float64(hf[H_PROGRESS, j]))
                if con and not con0:
                    if seen:
                        put(b, CONTACT_BEGIN, other=near, v0=clear)
                    self.contact_start[b], self.min_clearance[b], self.nearest[b] = t, clear, near
                elif con:
                    if clear < self.min_clearance[b]:
                        self.min_clearance[b] = clear
                    self.nearest[b] = near
                elif con0:
                    put(b, CONTACT_END, other=self.nearest[b], a=t - self.contact_start[b], v0=self.min_clearance[b])
                self.contact[b] = con
            else:
                self.contact[b] = 0
            if not self.contact[b]:
                self.nearest[b], self.contact_start[b], self.min_clearance[b] = -1, -1, 0.0
            if wf is not None:
                seen = self.seen_w[b] and not walls_fresh
                hit, imp = int(wi[W_HIT, b] != 0), wf[W_IMPULSE, b]
                hit0 = self.hit[b] if seen else 0
                if hit and not hit0:
                    if seen:
                        put(b, WALL_HIT, a=wi[W_SIDE, b], bb=wi[W_CORNER, b], v0=wf[W_DEPTH, b], v1=imp)
                    self.hit_start[b], self.max_impulse[b] = t, imp
                elif hit:
                    if imp > self.max_impulse[b]:
                        self.max_impulse[b] = imp
                elif hit0:
                    put(b, WALL_CLEAR, a=t - self.hit_start[b], v0=self.max_impulse[b])
                self.hit[b] = hit
            else:
                self.hit[b] = 0
            if not self.hit[b]:
                self.hit_start[b], self.max_impulse[b] = -1, 0.0
        # the before words, behind every vehicle's walk
        self.seen = True
        self.phase, self.lap = phase.copy(), lap.copy()
        for b in range(B):
            has_h = hf is not None and heat[b] >= 0
            self.seen_h[b] = has_h
            self.position[b] = hi[H_POSITION, b] if has_h else -1
            self.cls[b] = hi[H_CLASS, b] if has_h else -1
        self.seen_w[:] = wf is not None
        self.count_total += self.count
        self.total += len(out)
        return out


class Ring(object):
    """The ring: the event with global index g lives in slot g % capacity; a tick writes an event only when g >= total_after - capacity."""

    def __init__(self, capacity):
        self.capacity = int(capacity)
        self.slots = [None] * self.capacity
        self.total = 0
        self.writes = 0                                         # slot writes, for the rule "no two writes of one tick meet in a slot"

    def push_tick(self, events):
        n = len(events)
        after = self.total + n
        hit = set()
        for k, ev in enumerate(events):
            g = self.total + k
            if g >= after - self.capacity:
                assert g % self.capacity not in hit
                hit.add(g % self.capacity)
                self.slots[g % self.capacity] = ev
                self.writes += 1
        self.total = after

    @property
    def kept(self):
        return min(self.total, self.capacity)

    def read(self, n=None):
        """The last min(n, kept) events, oldest first."""
        m = self.kept if n is None else min(int(n), self.kept)
        return [self.slots[(self.total - m + j) % self.capacity] for j in range(m)]


def arrays(events):
    """Events -> (i32 [m, 6], f64 [m, 2])."""
    i = np.array([e[:6] for e in events], np.int32).reshape(-1, 6)
    f = np.array([e[6:] for e in events], np.float64).reshape(-1, 2)
    return i, f


def same_doubles(a, b):
    """Bit for bit, a NaN matching a NaN."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool(np.all((na == nb) & (na | (a.view(np.int64) == b.view(np.int64)))))


def assert_same(table, events, what=""):
    """A device table (events.events_table) against reference events: integers exactly, doubles bit for bit."""
    i, f = arrays(events)
    assert table.shape[0] == i.shape[0], (what, table.shape[0], i.shape[0])
    for c, k in enumerate(("tick", "kind", "vehicle", "other", "a", "b")):
        bad = np.nonzero(table[k] != i[:, c])[0]
        assert bad.size == 0, (what, k, int(bad[0]), table[bad[0]], events[bad[0]])
    for c, k in enumerate(("v0", "v1")):
        assert same_doubles(table[k], f[:, c]), (what, k)
