"""Numpy restatement of the heats (include/lpvmpc.h, "Heats"), written from the definitions, not from the kernel.

Two parts.  The order, turns, progress, gaps, passes and line crossings are float64 with the exact operation order (progress =
float64(turns) * L + s, product and sum each rounded; each gap one subtraction), so the device's words must equal them.  sep is
evaluated in numpy.longdouble, and every pair comes with its BAND, 32 * 2**-52 * (|dx| + |dy| + half_length + half_width_car): the
round-off that a float64 evaluation of the at most eight products and sums per axis, with a sincos good to 2 ulp, can carry.  The
device's sep is held to the band; a contact flag whose reference |sep| lies inside the band may go either way."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52


def sep_pair(pa, pb, hl, hw):
    """(sep, band) of two footprints, pa / pb = (x, y, yaw); pa is the first rectangle (the lower index)."""
    xa, ya, ta = (LD(v) for v in pa)
    xb, yb, tb = (LD(v) for v in pb)
    hl, hw = LD(hl), LD(hw)
    dx, dy = xb - xa, yb - ya
    gaps = []
    for th, oth in ((ta, tb), (tb, ta)):
        u = (np.cos(th), np.sin(th)); v = (-np.sin(th), np.cos(th))             # the rectangle's axes
        ou = (np.cos(oth), np.sin(oth)); ov = (-np.sin(oth), np.cos(oth))       # the other rectangle's
        for a, own in ((u, hl), (v, hw)):
            r_other = hl * abs(ou[0] * a[0] + ou[1] * a[1]) + hw * abs(ov[0] * a[0] + ov[1] * a[1])
            gaps.append(abs(dx * a[0] + dy * a[1]) - (own + r_other))
    band = 32 * EPS * (abs(float(dx)) + abs(float(dy)) + float(hl) + float(hw))
    return max(gaps), band


def sep_matrix(poses, hl, hw):
    """sep and band of every ordered pair of poses [n, 3] at once: entry [i, j] is the pair's sep with the lower index as the first
    rectangle, so the matrices are symmetric.  The same expressions as sep_pair, on longdouble arrays."""
    P = np.asarray(poses, LD)
    n = P.shape[0]
    x, y, th = P[:, 0], P[:, 1], P[:, 2]
    c, s = np.cos(th), np.sin(th)
    hl, hw = LD(hl), LD(hw)
    A, Bq = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")               # A first, Bq second
    dx, dy = x[Bq] - x[A], y[Bq] - y[A]
    best = None
    for own, oth in ((A, Bq), (Bq, A)):
        u = (c[own], s[own]); v = (-s[own], c[own])
        ou = (c[oth], s[oth]); ov = (-s[oth], c[oth])
        for a, ext in ((u, hl), (v, hw)):
            r_other = hl * np.abs(ou[0] * a[0] + ou[1] * a[1]) + hw * np.abs(ov[0] * a[0] + ov[1] * a[1])
            gap = np.abs(dx * a[0] + dy * a[1]) - (ext + r_other)
            best = gap if best is None else np.maximum(best, gap)
    up = np.triu(np.ones((n, n), bool), 1)
    sep = np.where(up, best, best.T)
    band = 32 * EPS * (np.abs(dx).astype(float) + np.abs(dy).astype(float) + float(hl) + float(hw))
    return sep, band


def corners(p, hl, hw):
    x, y, th = (float(v) for v in p)
    c, s = np.cos(th), np.sin(th)
    return [(x + sx * hl * c - sy * hw * s, y + sx * hl * s + sy * hw * c) for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1))]


def polygons_intersect(P, Q):
    """Brute force: an edge of P crosses or touches an edge of Q, or one polygon holds a vertex of the other (convex polygons)."""
    def orient(a, b, c):
        return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])

    def seg(a, b, c, d):
        o1, o2, o3, o4 = orient(a, b, c), orient(a, b, d), orient(c, d, a), orient(c, d, b)
        return (o1 > 0) != (o2 > 0) and (o3 > 0) != (o4 > 0)

    def inside(pt, R):
        sg = [orient(R[k], R[(k + 1) % len(R)], pt) for k in range(len(R))]
        return all(v >= 0 for v in sg) or all(v <= 0 for v in sg)

    for k in range(len(P)):
        for m in range(len(Q)):
            if seg(P[k], P[(k + 1) % len(P)], Q[m], Q[(m + 1) % len(Q)]):
                return True
    return any(inside(pt, Q) for pt in P) or any(inside(pt, P) for pt in Q)


def _nan_eq(a, b):
    return (a == b) or (a != a and b != b)


class HeatsRef(object):
    """The heats of B vehicles, stepped on the host.  heat [B] (-1: none), L [B] or one value, turns0 [B] or None, phase0 [B] the
    phases before the attach (None: running), lines = K columns of the line tables."""

    def __init__(self, heat, L, turns0=None, phase0=None, half_length=0.4, half_width=0.2, lines=0):
        self.heat = np.asarray(heat, int)
        B = self.B = self.heat.shape[0]
        self.L = np.broadcast_to(np.asarray(L, float), (B,)).copy()
        self.hl, self.hw = float(half_length), float(half_width)
        self.turns0 = np.zeros(B, int) if turns0 is None else np.asarray(turns0, int).copy()
        self.turns = self.turns0.copy()
        self.located = np.zeros(B, bool)
        self.s_last = np.zeros(B)
        self.progress = np.full(B, np.nan)
        self.cls = None                                         # classes of the previous tick (None: no tick yet)
        self.phase_prev = np.zeros(B, int) if phase0 is None else np.asarray(phase0, int).copy()
        self.finish = np.full(B, -1, int)
        self.crossings = np.zeros(B, int)
        self.min_clearance = np.full(B, np.inf)
        self.min_band = np.zeros(B)                             # the largest band of any tick so far: what min_clearance is held to
        self.contact_ticks = np.zeros(B, int)
        self.first_contact = np.full(B, -1, int)
        self.passes = np.zeros(B, int)
        self.passed = np.zeros(B, int)
        self.K = int(lines)
        self.line_tick = np.full((B, self.K), -1, int)
        self.line_pos = np.full((B, self.K), -1, int)
        self.members = {int(g): np.nonzero(self.heat == g)[0] for g in np.unique(self.heat[self.heat >= 0])}

    @staticmethod
    def order_key(cls, finish, progress, idx):
        nan = progress != progress
        return (cls, finish if cls == 0 else 0, 1 if nan else 0, 0.0 if nan else -progress, idx)

    def step(self, t, pose, s, inside, phase):
        """One tick.  Returns a dict of [B] arrays: the standings' channels, plus band (the band of the pair that gives the
        clearance, the largest band of the vehicle's pairs) and ambiguous (the reference |clearance| is inside that band, or the
        nearest partner is not clear of the second nearest by their bands)."""
        pose = np.asarray(pose, float); s = np.asarray(s, float); inside = np.asarray(inside, int); phase = np.asarray(phase, int)
        B = self.B
        in_heat = self.heat >= 0
        prev_prog, prev_cls = self.progress.copy(), None if self.cls is None else self.cls.copy()
        for b in np.nonzero(in_heat)[0]:
            if inside[b] == 1 and np.isfinite(s[b]):
                if self.located[b]:
                    d = s[b] - self.s_last[b]
                    if d < -self.L[b] / 2:
                        self.turns[b] += 1
                    elif d > self.L[b] / 2:
                        self.turns[b] -= 1
                self.s_last[b] = s[b]
                self.located[b] = True
            if self.located[b]:
                tl = np.float64(self.turns[b]) * np.float64(self.L[b])
                self.progress[b] = tl + self.s_last[b]
            if phase[b] == 2 and self.phase_prev[b] != 2:
                self.finish[b] = t
        cls = np.where(phase == 2, 0, np.where(phase == 3, 3, np.where(self.located, 1, 2)))
        cls = np.where(in_heat, cls, -1)
        out = dict(progress=np.where(in_heat, self.progress, np.nan), gap_ahead=np.full(B, np.nan), gap_leader=np.full(B, np.nan),
                   clearance=np.full(B, np.nan), min_clearance=np.full(B, np.nan), position=np.full(B, -1, int), ahead=np.full(B, -1, int),
                   nearest=np.full(B, -1, int), contact=np.zeros(B, int), band=np.zeros(B), ambiguous=np.zeros(B, bool))
        for g, mem in self.members.items():
            order = sorted(mem, key=lambda b: self.order_key(cls[b], self.finish[b], self.progress[b], b))
            for p, b in enumerate(order):
                out["position"][b] = p
                if p > 0:
                    a, lead = order[p - 1], order[0]
                    out["ahead"][b] = a
                    if cls[b] == 1 and cls[a] == 1:
                        out["gap_ahead"][b] = self.progress[a] - self.progress[b]
                    if cls[b] == 1 and cls[lead] == 1:
                        out["gap_leader"][b] = self.progress[lead] - self.progress[b]
            # passes: pairs that are class 1 on the previous tick and on this one
            if prev_cls is not None:
                both = [b for b in mem if cls[b] == 1 and prev_cls[b] == 1]
                for i in both:
                    for j in both:
                        if i == j:
                            continue
                        i_was_behind = self.order_key(1, 0, prev_prog[j], j) < self.order_key(1, 0, prev_prog[i], i)
                        i_in_front = out["position"][i] < out["position"][j]
                        if i_was_behind and i_in_front:
                            self.passes[i] += 1
                            self.passed[j] += 1
            # line crossings
            for b in mem:
                if self.turns[b] - self.turns0[b] > self.crossings[b]:
                    k = self.crossings[b]
                    self.crossings[b] += 1
                    if k < self.K:
                        self.line_tick[b, k] = t
                        self.line_pos[b, k] = out["position"][b]
            # clearances
            elig = np.array([b for b in mem if cls[b] in (1, 2) and np.all(np.isfinite(pose[b]))], int)
            sep, band = sep_matrix(pose[elig], self.hl, self.hw) if elig.size > 1 else (None, None)
            for i in mem:
                best, near, bmax, amb = LD(np.inf), -1, 0.0, False
                w = np.nonzero(elig == i)[0]
                if w.size and elig.size > 1:
                    k = int(w[0])
                    row = sep[k].copy(); row[k] = LD(np.inf)
                    m = int(np.argmin(row))                                     # (the first of equal minima: the lowest index)
                    best, near, bnear = row[m], int(elig[m]), band[k, m]
                    others = np.ones(elig.size, bool); others[[k, m]] = False
                    bmax = float(np.max(np.where(np.arange(elig.size) == k, 0.0, band[k])))
                    close = others & (row - best <= band[k] + bnear) & ~np.all(pose[elig] == pose[elig[m]], axis=1)
                    amb = bool(abs(best) <= bnear or close.any())
                out["clearance"][i] = float(best)
                out["nearest"][i] = near
                out["band"][i] = bmax
                out["ambiguous"][i] = amb
                out["contact"][i] = int(best < 0)
                if best < self.min_clearance[i]:
                    self.min_clearance[i] = float(best)
                self.min_band[i] = max(self.min_band[i], bmax)
                self.contact_ticks[i] += int(best < 0)
                if best < 0 and self.first_contact[i] < 0:
                    self.first_contact[i] = t
        self.cls = cls
        self.phase_prev = np.where(in_heat, phase, self.phase_prev)
        z = lambda a, fill: np.where(in_heat, a, fill)
        out.update(min_clearance=z(self.min_clearance, np.nan), contact_ticks=z(self.contact_ticks, 0),
                   first_contact_tick=z(self.first_contact, -1), passes=z(self.passes, 0), passed=z(self.passed, 0), turns=z(self.turns, 0),
                   line_tick=self.line_tick.copy(), line_pos=self.line_pos.copy(), min_band=self.min_band.copy())
        out["class"] = cls
        return out


EXACT_I32 = ("position", "ahead", "turns", "class", "passes", "passed")
EXACT_F64 = ("progress", "gap_ahead", "gap_leader")


def same_words(a, b):
    """Word for word, a NaN matching a NaN."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool(np.all((na == nb) & (na | (a.view(np.int64) == b.view(np.int64)))))


def compare(dev, ref, what="", exact_sep=False, skip_contact=None):
    """The device's standings against the reference's: the order, progress, gaps, passes and turns word for word; the clearances
    within the band (``exact_sep``: word for word, for inputs whose sep is exact in float64); nearest and the contact flags equal
    where the reference is not ambiguous.  ``skip_contact`` [B] bool: vehicles whose cumulative contact counters are not compared
    (an earlier tick of theirs was ambiguous).  Prints nothing; raises AssertionError naming the first difference."""
    for k in EXACT_I32:
        assert np.array_equal(np.asarray(dev[k]), np.asarray(ref[k])), (what, k, np.asarray(dev[k]).tolist(), np.asarray(ref[k]).tolist())
    for k in EXACT_F64:
        assert same_words(dev[k], ref[k]), (what, k, np.asarray(dev[k]).tolist(), np.asarray(ref[k]).tolist())
    amb = np.asarray(ref["ambiguous"], bool)
    skip = amb.copy() if skip_contact is None else (np.asarray(skip_contact, bool) | amb)
    for k in ("clearance", "min_clearance"):
        d, r = np.asarray(dev[k], float), np.asarray(ref[k], float)
        assert np.array_equal(np.isnan(d), np.isnan(r)) and np.array_equal(np.isinf(d), np.isinf(r)), (what, k, d.tolist(), r.tolist())
        fin = np.isfinite(r)
        if exact_sep:
            assert same_words(d, r), (what, k, d.tolist(), r.tolist())
        else:
            bd = np.asarray(ref["band" if k == "clearance" else "min_band"])
            assert np.all(np.abs(d[fin] - r[fin]) <= bd[fin]), (what, k, np.abs(d[fin] - r[fin]).max(), bd[fin].max())
    ok = ~amb
    assert np.array_equal(np.asarray(dev["nearest"])[ok], np.asarray(ref["nearest"])[ok]), (what, "nearest")
    assert np.array_equal(np.asarray(dev["contact"])[ok], np.asarray(ref["contact"])[ok]), (what, "contact")
    ok = ~skip
    for k in ("contact_ticks", "first_contact_tick"):
        assert np.array_equal(np.asarray(dev[k])[ok], np.asarray(ref[k])[ok]), (what, k)
    if "line_tick" in dev and dev["line_tick"] is not None and ref["line_tick"].shape[1]:
        assert np.array_equal(dev["line_tick"], ref["line_tick"]), (what, "line_tick", dev["line_tick"].tolist(), ref["line_tick"].tolist())
        assert np.array_equal(dev["line_pos"], ref["line_pos"]), (what, "line_pos")
